# The emulator driver of CZ_COMPRESS_HIGH, under the flags and dependencies of the Makefile next to it:
# make -C tests/emu -f high.mk emu_encode_high
include Makefile
emu_encode_high: %: %.cpp $(DEPS) high.mk
	$(COMPILE) -o $@ $<
