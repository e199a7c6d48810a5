# The emulator driver of CZ_COMPRESS_HIGH_SPLIT, under the flags and dependencies of the Makefile next to it, with one-block segments
# and an 8 KiB overlap as emu_encode_split has them: make -C tests/emu -f high_split.mk emu_encode_high_split
include Makefile
emu_encode_high_split: DEFS := -DCZE_SEG_BLOCKS=1u -DCZE_OVERLAP=8192u
emu_encode_high_split: %: %.cpp $(DEPS) high_split.mk
	$(COMPILE) -o $@ $<
