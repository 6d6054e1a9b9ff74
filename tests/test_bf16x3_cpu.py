"""CPU-only checks of the bf16x3 training precision's host side (include/gm2.h GM2_BF16X3): the
constant and its header value, the workspace layout (the GM2_F32 layout plus the split operand
buffers), the GM2_OPT_TRAIN_SPLIT option, the GM2_TSTAT_* counter keys, the CLI flag and, with the
debug build, the layout's region checks."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gm2.h")).read()


def test_precision_constant_matches_header():
    from gm2 import native
    assert native.GM2_BF16X3 == 2
    m = re.search(r"enum \{ GM2_F32 = (\d+), GM2_BF16 = (\d+), GM2_BF16X3 = (\d+) \};", _header())
    assert m and [int(v) for v in m.groups()] == [native.GM2_F32, native.GM2_BF16, native.GM2_BF16X3]
    # additive: the ABI version does not move
    assert native.lib().gm2_abi_version() == 6


def test_workspace_size_and_bad_precision():
    from gm2 import native
    d = native.dims(55039, 1024, 64, 4096)
    x3 = native.workspace_size(d, native.GM2_BF16X3)
    f32 = native.workspace_size(d, native.GM2_F32)
    assert x3 >= f32
    # the split buffers at this shape: W0, 2 x W9, (x | x), x, 2 x A5, 2 x dL, dY0 in bf16 + the row table
    Gq, Bq, H = 55040, 4096, 1024
    extra = 2 * (3 * 2 * Gq * H + 3 * Bq * Gq + 2 * 2 * Bq * Gq + 3 * 2 * Bq * H) + 4 * 2 * Bq
    assert x3 - f32 == extra
    with pytest.raises(RuntimeError, match="bad precision"):
        native.workspace_size(d, 3)
    # the small shape of the GPU tests
    assert native.workspace_size(native.dims(700, 128, 16, 96), native.GM2_BF16X3) > \
        native.workspace_size(native.dims(700, 128, 16, 96), native.GM2_F32)


def test_train_split_option():
    from gm2 import native
    assert native.OPT_TRAIN_SPLIT == 24
    assert native.get_option(native.OPT_TRAIN_SPLIT) == 1
    native.set_option(native.OPT_TRAIN_SPLIT, 0)
    assert native.get_option(native.OPT_TRAIN_SPLIT) == 0
    native.set_option(native.OPT_TRAIN_SPLIT, 1)
    assert native.get_option(native.OPT_TRAIN_SPLIT) == 1
    with pytest.raises(RuntimeError, match="train split"):
        native.set_option(native.OPT_TRAIN_SPLIT, 2)
    assert native.get_option(native.OPT_TRAIN_SPLIT) == 1


def test_train_stat_keys():
    from gm2 import native
    txt = _header()
    keys = dict((k, int(v)) for k, v in re.findall(r"GM2_TSTAT_([A-Z_]+) = (\d+)", txt))
    assert keys == {"SPLIT_GEMMS": 32, "EXACT_GEMMS": 33}
    assert native.TRAIN_STATS == {"split_gemms": 32, "exact_gemms": 33}
    assert (native.TSTAT_SPLIT_GEMMS, native.TSTAT_EXACT_GEMMS) == (32, 33)
    # (read through gm2_workspace_stat: a workspace libgm2 never initialised is refused)
    v = ctypes.c_int64()
    assert native.lib().gm2_workspace_stat(ctypes.c_void_p(0x1000), native.TSTAT_SPLIT_GEMMS, ctypes.byref(v)) != 0
    assert "not initialised" in native.lib().gm2_last_error().decode()
    assert "gm2_split_operand" in native.EXPORTS


def test_cli_parses_bf16x3():
    import main
    args = main.parse_arguments(["--precision", "bf16x3"])
    assert args.precision == "bf16x3"
    assert "bf16x3" in main.PRECISION_NOTE
    from gm2 import native
    assert main._precision(args) == native.GM2_BF16X3
    assert main._precision(main.parse_arguments(["--precision", "f32"])) == native.GM2_F32
    assert main._precision(main.parse_arguments([])) == native.GM2_BF16


def test_debug_layout_check():
    """gm2_debug_check_layout (debug build): every region of the new precision's layout is aligned,
    disjoint and inside the total, and the split buffers are named regions."""
    import subprocess
    import sys
    debug_lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(debug_lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    # a child process with GM2_LIB_PATH set, so this process keeps the release library
    code = """
import ctypes, sys
sys.path.insert(0, 'genome-minimizer-2_amd')
from gm2 import native
L = native.lib()
for shape in ((55039, 1024, 64, 4096), (700, 128, 16, 96)):
    d = native.dims(*shape)
    n, total = ctypes.c_int64(), ctypes.c_int64()
    rc = L.gm2_debug_check_layout(ctypes.byref(d), native.GM2_BF16X3, ctypes.byref(n), ctypes.byref(total))
    assert rc == 0, L.gm2_last_error().decode()
    assert total.value == native.workspace_size(d, native.GM2_BF16X3) > native.workspace_size(d, native.GM2_F32)
    assert n.value > 60
assert L.gm2_debug_check_layout(ctypes.byref(d), 3, ctypes.byref(n), ctypes.byref(total)) != 0
assert 'bad precision' in L.gm2_last_error().decode()
print('LAYOUT_OK')
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, GM2_LIB_PATH=debug_lib),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LAYOUT_OK" in r.stdout, r.stdout + r.stderr
