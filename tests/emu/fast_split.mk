# The emulator driver of CZ_COMPRESS_FAST_SPLIT, under the flags and dependencies of the Makefile next to it:
# make -C tests/emu -f fast_split.mk emu_encode_fast_split
include Makefile
emu_encode_fast_split: %: %.cpp $(DEPS) fast_split.mk
	$(COMPILE) -o $@ $<
