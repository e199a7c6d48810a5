"""Runs the kernel source on the CPU SIMT emulator (tests/emu) — sanitizer coverage for the
HIP kernels without a GPU.  Test infrastructure only."""
import emu_common
from emu_common import EMU_DIR, RESULT_DTYPE  # noqa: F401  (re-exported)


def build(target="emu_decode"):
    return emu_common.build(target)


def run(frames, caps, target="emu_decode", timeout=900, chain_bytes=0, exec_kernel=False, lit_bytes=0, dict_path=None, wexec_waves=0, verify=True, wexec_auto=False, debug_flags=0):
    env = dict(EMU_CHAIN=str(int(chain_bytes)), EMU_EXEC="1" if exec_kernel else "0", EMU_LIT=str(int(lit_bytes)),
               EMU_VERIFY="1" if verify else "0", EMU_DEBUG_FLAGS=str(int(debug_flags)))
    if dict_path:
        env["EMU_DICT"] = dict_path
    if wexec_waves:
        env["EMU_WEXEC"] = str(int(wexec_waves))
        if wexec_auto:
            env["EMU_WX_AUTO"] = "1"
    raw, run.last_stderr = emu_common.execute(target, emu_common.decode_batch(frames, caps), timeout, **env)
    return emu_common.results(raw[0], 0, RESULT_DTYPE, caps, produced="bytes_produced")
