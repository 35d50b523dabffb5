"""The shared level scheduler (elliot_amd/csrc/el_levels.h): its stand-alone check under AddressSanitizer and UBSan on the host,
both entry points against the arrays they returned before they shared it (tests/golden/levels_parent.npz: 4 000 random triplets
over 40 users x 60 items, 70 of them with i == j, recorded from ops.sgd_levels and ops.bprslim_levels of the commit before the
merge), and -- on the GPU -- el_bprsgd_apply_levels refusing a malformed level table before it launches anything."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_levels_header_under_asan_and_ubsan(tmp_path):
    """tests/host/levels_check.cpp is a program of its own: nothing is loaded into Python and nothing is preloaded."""
    exe = str(tmp_path / "levels_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "elliot_amd", "csrc"),
                           os.path.join(REPO, "tests", "host", "levels_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout


def test_both_schedulers_return_what_they_returned_before_the_merge(golden):
    from elliot_amd import ops
    g = golden("levels_parent.npz")
    u, i, j, (U, I) = g["u"], g["i"], g["j"], g["sizes"]
    assert len(u) == 4000 and (i == j).sum() == 70
    for (order, start), tag in ((ops.sgd_levels(u, i, j, U, I), "sgd"), (ops.bprslim_levels(i, j, I), "bprslim")):
        assert order.dtype == np.int32 and start.dtype == np.int64
        assert np.array_equal(order, g[f"{tag}_order"]) and np.array_equal(start, g[f"{tag}_start"]), tag


def test_sgd_levels_edges_and_messages():
    from elliot_amd import _lib, ops
    order, start = ops.sgd_levels(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 3, 4)
    assert len(order) == 0 and start.tolist() == [0]
    order, start = ops.sgd_levels([1, 0, 1], [0, 1, 2], [2, 3, 3], 2, 4)     # user 1 and item 1 are different rows
    assert order.tolist() == [0, 1, 2] and start.tolist() == [0, 2, 3]
    with pytest.raises(_lib.ElliotHipError, match="el_bprsgd_levels_host: triplet 1 out of range"):
        ops.sgd_levels([0, 2], [0, 1], [1, 2], 2, 4)
    with pytest.raises(_lib.ElliotHipError, match="el_bprslim_levels_host: triplet 2 out of range"):
        ops.bprslim_levels([0, 1, 2], [1, 2, -1], 4)
    lib, three = _lib.load(), (C.c_int32 * 3)(0, 0, 0)
    order, start, nl = (C.c_int32 * 3)(), (C.c_int64 * 3)(), C.c_int64()
    for rc in (lib.el_bprsgd_levels_host(three, three, three, 3, 1, 1, order, start, 3, C.byref(nl)),
               lib.el_bprslim_levels_host(three, three, 3, 1, order, start, 3, C.byref(nl))):
        assert rc == 2 and "3 levels exceed capacity 3" in lib.el_last_error().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("starts", [[0, 2, 1, 4], [0, 2, -1, 4]], ids=["b_below_a", "a_negative"])
def test_bprsgd_apply_levels_refuses_a_malformed_table_before_launching(ctx, starts):
    """The second level is [2, 1) or [-1, 4): the call fails and the first, well-formed level has not run either."""
    import torch
    from elliot_amd import _lib, ops
    rs = np.random.RandomState(3)
    P, Q, b = rs.normal(size=(4, 8)), rs.normal(size=(6, 8)), rs.normal(size=6)
    st = ops.BprSgdDeviceState(ctx, P, Q, b, lr=0.5, reg_bias=0.0, reg_user=0.0025, reg_pos=0.0025, reg_neg=0.00025)
    u, i, j = (torch.tensor(x, dtype=torch.int32, device=ctx.device) for x in ([0, 1, 2, 3], [0, 2, 4, 1], [1, 3, 5, 0]))
    table = np.asarray(starts, dtype=np.int64)
    args = (ctx.handle, ctx.stream(), C.byref(st._c), ops._ptr(u), ops._ptr(i), ops._ptr(j), table.ctypes.data_as(C.c_void_p))
    with pytest.raises(_lib.ElliotHipError, match=r"el_bprsgd_apply_levels: level 1 is \[%d, %d\)" % (starts[1], starts[2])):
        ops.check(ctx.lib.el_bprsgd_apply_levels(*args, 3), "el_bprsgd_apply_levels")
    torch.cuda.synchronize()
    for got, ref in ((st.P, P), (st.Q, Q), (st.b, b)):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    ops.check(ctx.lib.el_bprsgd_apply_levels(*args, 1), "el_bprsgd_apply_levels")          # the well-formed level alone runs
    torch.cuda.synchronize()
    assert not np.array_equal(st.P.cpu().numpy(), P)
