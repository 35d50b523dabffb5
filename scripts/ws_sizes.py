"""Print every workspace size query of the library on a fixed set of shapes, one line per call.

Two builds lay their workspaces out alike when their outputs are equal:
    EL_LIB_PATH=<other build>/libelliot_hip.so python scripts/ws_sizes.py > a.txt;  python scripts/ws_sizes.py > b.txt;  cmp a.txt b.txt
Without --gpu only the queries that need no device are printed; with it, also the ones that ask rocprim for a size."""
import itertools
import math
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from elliot_amd import _lib  # noqa: E402

EDGE = [0, 1, 2, 63, 64, 65, 255, 257]


def shapes(rs, n, *ranges):
    """The cross product of the edge values that fit each range, cut to n, then random draws up to n shapes in all."""
    edge = list(itertools.product(*[[v for v in EDGE if lo <= v <= hi] + [hi] for lo, hi in ranges]))
    rs.shuffle(edge)
    out = edge[: n // 2]
    while len(out) < n:                                       # log-uniform: small and large sizes alike
        out.append(tuple(min(hi, lo + int(math.exp(rs.uniform(0, math.log(hi - lo + 1)))) - 1) for lo, hi in ranges))
    return out


def main():
    if "--gpu" in sys.argv:
        from elliot_amd import ops                            # (torch's HIP runtime first, as everywhere else)
        lib = ops.get_context(0).lib                          # rocprim's size queries want a bound device
    else:
        lib = _lib.load()
    rs = random.Random(20260)
    N = 320
    cpu = {
        "el_knn_ws_bytes": shapes(rs, N, (0, 200000), (0, 900)),                        # n_neighbors > n among them
        "el_rp3_ws_bytes": shapes(rs, N, (0, 200000), (0, 900), (0, 5000)),
        "el_slim_ws_bytes": shapes(rs, N, (0, 200000), (0, 60000), (0, 64), (0, 400)),  # both placements: U * 4 around the LDS limit
        "el_psvd_orth_ws_bytes": shapes(rs, N, (0, 3000000), (0, 256)),
        "el_gram_f64_ws_bytes": shapes(rs, N, (0, 3000000), (0, 256)),
        "el_psvd_signs_ws_bytes": shapes(rs, N, (0, 3000000), (0, 256)),
        "el_bpr_sample_mt19937_ws_bytes": shapes(rs, N, (0, 1 << 26)),
        "el_rec_metrics_ws_bytes": shapes(rs, N, (0, 9000000)),
        "el_beyond_ws_bytes": [(u, 0) for (u,) in shapes(rs, N, (0, 9000000))],          # (n_items > 0 asks rocprim: --gpu)
        "el_lightgcn_ws_bytes": [s + (l,) for l in (0, 1, 2, 3, 4) for s in shapes(rs, N // 4, (0, 500000), (0, 500000), (1, 256))],
        "el_score_topk_ws_bytes": [s + (a,) for a in (0, 3) for s in
                                   shapes(rs, N // 2, (0, 200000), (0, 1000000), (1, 256), (1, 128), (0, 5000000))],
        "el_bprmf_train_loop_ws_bytes": shapes(rs, N, (0, 30000000), (0, 2000000)),
        "el_pwmf_train_loop_ws_bytes": shapes(rs, N, (0, 30000000), (0, 2000000)),
        "el_knn_f32_ws_bytes": shapes(rs, N, (0, 200000), (0, 900)),
        "el_profile_ws_bytes": shapes(rs, N, (0, 9000000)),
    }
    slim = cpu["el_slim_ws_bytes"]
    slim += [(38000, 3706, c, 10) for c in (0, 1, 2, 9)] + [(37000, 3706, c, 10) for c in (1, 2)] + [(138493, 26744, 9, 10)]
    gpu = {
        "el_bprmf_ws_bytes": [(0, 10, 10, 8), (1, 1, 2, 1), (777, 300, 1000, 64), (2048, 6040, 3706, 64), (1 << 20, 1000003, 50021, 128)],
        "el_pwmf_ws_bytes": [(0, 10, 10, 8), (1, 1, 2, 1), (777, 300, 1000, 64), (4096, 6040, 3706, 10), (1 << 20, 1000003, 50021, 128)],
        "el_cml_ws_bytes": [(0, 0, 10, 10, 8), (1, 1, 1, 2, 1), (777, 3108, 300, 1000, 64), (4096, 4096, 6040, 3706, 100)],
        "el_rows_segment_sum_ws_bytes": [(0, 10), (1, 1), (777, 300), (1 << 20, 1000003)],
        "el_beyond_ws_bytes": [(257, 301), (0, 5001), (100000, 3706), (5, 1 << 22)],
    }
    if "--gpu" in sys.argv:
        cpu.update({k + " ": v for k, v in gpu.items()})
    for name, cases in cpu.items():
        fn = getattr(lib, name.strip())
        for args in cases:
            print(name.strip(), *args, "->", int(fn(*args)))


if __name__ == "__main__":
    main()
