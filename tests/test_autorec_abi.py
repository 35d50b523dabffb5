"""el_autorec_state of include/elliot_hip.h against its ctypes mirror elliot_amd/_lib.py::AutoRecState: same size, every field at the
same offset (a C program built from the header prints offsetof / sizeof), in the manner of
tests/test_abi.py::test_ctypes_structs_match_the_header_layout."""
import ctypes
import os
import shutil
import subprocess

import pytest

from elliot_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_autorec_state_matches_the_header_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    cname, cls = "el_autorec_state", _lib.AutoRecState
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elliot_hip.h"', "int main(void) {",
             f'    printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'    printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _ in cls._fields_]
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[cname]) == ctypes.sizeof(cls), (out[cname], ctypes.sizeof(cls))
    for fname, _ in cls._fields_:
        assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    assert [f for f, _ in cls._fields_] == ["N", "H", "out_act", "Bmax", "nnz_max", "w", "g", "m", "v", "h", "dh", "d", "ws", "ws_bytes"]


def test_autorec_entry_points_are_bound():
    for name in ("el_autorec_ws_bytes", "el_autorec_grads", "el_autorec_apply", "el_autorec_train_step", "el_autorec_encode",
                 "el_autorec_rowbias_act"):
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.el_abi_version() == 8
    assert lib.el_autorec_ws_bytes(203, 150, 1000) > 4 * (4 * 204 + 151 + 1000)
    assert lib.el_autorec_ws_bytes(0, 150, 1000) == 0
