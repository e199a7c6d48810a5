# The seekable-read drivers, under the flags and dependencies of the Makefile next to it:
#   make -C tests/emu -f seekable_read.mk emu_seekable_read          the kernels of czstd_seekable_read.hip on the emulator
#   make -C tests/emu -f seekable_read.mk seekable_read_host_main    czstd_seekable_read_host.h alone: g++, no HIP, no emulator header
include Makefile
emu_seekable_read: %: %.cpp $(DEPS) seekable_read_cases.h seekable_read.mk
	$(COMPILE) -o $@ $<
seekable_read_host_main: %: %.cpp $(SRC)/czstd_seekable_read_host.h $(SRC)/czstd_seekable_host.h $(ROOT)/include/cairo_zstd_amd.h $(ROOT)/include/cairo_zstd_amd_status.h seekable_read_cases.h seekable_read.mk
	$(CXX) -std=c++17 $(SAN) -g -Wall -I$(ROOT)/include -I$(SRC) -o $@ $<
