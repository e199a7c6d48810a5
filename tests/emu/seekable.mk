# The seekable-stream drivers, under the flags and dependencies of the Makefile next to it:
#   make -C tests/emu -f seekable.mk emu_seekable          the kernels of czstd_seekable.hip on the emulator
#   make -C tests/emu -f seekable.mk seekable_host_main    czstd_seekable_host.h alone: g++, no HIP, no emulator header
include Makefile
emu_seekable: %: %.cpp $(DEPS) seekable_cases.h seekable.mk
	$(COMPILE) -o $@ $<
seekable_host_main: %: %.cpp $(SRC)/czstd_seekable_host.h $(ROOT)/include/cairo_zstd_amd.h $(ROOT)/include/cairo_zstd_amd_status.h seekable_cases.h seekable.mk
	$(CXX) -std=c++17 $(SAN) -g -Wall -I$(ROOT)/include -I$(SRC) -o $@ $<
