"""The stdout line of bench.py stays one a consumer with a bounded read can parse (round 4's 22 KB line came back `parsed: null` from
the driver): compact_line() applied to the fattest report on record -- the committed round-4 line with every leg -- is strict JSON,
below the limit, and still carries the contract's fields, `roofline` and `cpu_baseline`.  (CPU; the GPU contract test checks the same
on a live run.)"""
import importlib.util
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_line_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _strict(text):
    def bad(c):
        raise ValueError(c)
    return json.loads(text, parse_constant=bad)


def test_compact_line_of_the_fattest_report_is_small_strict_and_complete():
    b = _bench()
    full = json.load(open(os.path.join(REPO, "profiles", "r04_n_bench_line.json")))
    assert len(json.dumps(full)) > 20000                       # the report that broke the consumer
    full["roofline"]["traffic"] = 5.14e9                       # + the stamps a traffic file adds
    full["topk"]["roofline"]["traffic"] = float("nan")         # + a non-finite float somewhere
    text = json.dumps(b.compact_line(full), allow_nan=False, separators=(",", ":"))
    assert len(text.encode()) <= b.LINE_LIMIT <= 6144, len(text)
    d = _strict(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline", "topk_users_per_s", "topk_ms_per_block", "topk_frac"):
        assert key in d, key
    assert "10M users x 1M items" in d["config"]["workload"] and "model" not in d["config"]
    r = d["roofline"]
    assert set(("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r) and r["traffic"] == 5.14e9 and "builder" in d["traffic_source"]
    assert d["topk"]["roofline"]["traffic"] is None            # NaN -> null
    assert not any(k.endswith("GBs") and isinstance(v, float) and v > r["peak"] for k, v in r.items())
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 16 and cb["value"] > 0 and cb["topk"]["value"] > 0 and cb["sample"]
    assert set(d["legs"]) == {"c2", "c5_per_gpu", "batch_sweep", "plugin_e2e", "vae", "neumf"}
    assert d["legs"]["vae"]["roofline"]["kernel"] == "k_gemm_b3" and d["legs"]["neumf"]["topk"]["roofline"]["kernel"] == "k_nmf_screen"


def test_emit_drops_summaries_rather_than_exceed_the_limit(tmp_path, capsys):
    b = _bench()
    full = json.load(open(os.path.join(REPO, "profiles", "r04_n_bench_line.json")))
    full["batch_sweep"]["points"] = full["batch_sweep"]["points"] * 40           # a leg that would blow the line up
    args = type("A", (), {"legs_file": str(tmp_path / "legs.json")})()
    b.emit(full, args)
    out = capsys.readouterr().out.rstrip().splitlines()
    assert len(out) == 1 and len(out[0].encode()) <= b.LINE_LIMIT
    d = _strict(out[0])
    assert "legs" not in d and d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0
    kept = _strict(open(tmp_path / "legs.json").read())
    assert len(kept["batch_sweep"]["points"]) == 240                             # the side file keeps everything


def test_plain_report_line_carries_the_headline_only(capsys):
    """A plain run's report (no --full: no roofline, no top-k, no legs) prints the contract's fields and nothing it did not measure,
    and writes no side file."""
    b = _bench()
    full = {"metric": "BPR-MF positive-pairs/sec + full-catalog top-k users/sec", "value": 7.0e8, "unit": "pairs/s", "n_gpus": 1,
            "steps": 5, "warmup": 2, "ms_per_step": 1.5, "repeats_ms_per_step": [1.5], "repeats": 1, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": False,
            "config": {"workload": "BPRMF d=128", "users": 10, "items": 5, "factors": 128, "batch": 1 << 20, "topk_block": None, "k": None},
            "loss_per_pair_last": 0.69}
    b.emit(full, type("A", (), {"legs_file": None, "full": False})())
    out = capsys.readouterr().out.rstrip().splitlines()
    d = _strict(out[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert d[key] == full[key], key
    assert d["full"] is False and "topk_block" not in d["config"] and "k" not in d["config"]
    for key in ("roofline", "topk", "legs", "cpu_baseline", "legs_file"):
        assert key not in d, key


def test_plain_run_refuses_legs_without_full(monkeypatch, capsys):
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--legs", "bpr,vae"])
    try:
        b.parse()
        raise AssertionError("parse() accepted --legs without --full")
    except SystemExit as ex:
        assert ex.code == 2 and "--full" in capsys.readouterr().err
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--legs", "bpr,vae", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full and a.legs == "bpr,vae" and a.dump_outputs == "out"
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "7"])
    a = b.parse()
    assert not a.full and a.steps == 7 and a.dump_outputs is None


def test_dumped_outputs_are_a_fixed_sample_within_the_limit(tmp_path):
    """train_outputs: tables up to OUTPUT_TABLE_BYTES whole, larger ones as the same seeded rows every time; float32 / float64 only;
    write_outputs refuses more than 64 MB."""
    import numpy as np
    import torch
    b = _bench()
    F = 128
    big = b.OUTPUT_TABLE_BYTES // (4 * F) * 3 + 5
    st = type("S", (), {"Gu": torch.arange(big * F, dtype=torch.float32).view(big, F), "Gi": torch.ones((1000, F)),
                        "Bi": torch.zeros(1000)})()
    o1, o2 = b.train_outputs(st, 0.5), b.train_outputs(st, 0.5)
    assert set(o1) == {"loss_per_pair", "Gu", "Gu_rows", "Gi", "Bi"} and o1["loss_per_pair"].tolist() == [0.5]
    rows = o1["Gu_rows"].astype(np.int64)
    assert len(rows) == b.OUTPUT_TABLE_BYTES // (4 * F) and (np.diff(rows) > 0).all() and rows[-1] < big
    assert np.array_equal(o1["Gu"], st.Gu.numpy()[rows]) and o1["Gi"].shape == (1000, F) and o1["Bi"].shape == (1000,)
    assert all(np.array_equal(o1[k], o2[k]) for k in o1)
    assert all(a.dtype in (np.float32, np.float64) for a in o1.values())
    b.write_outputs(o1, str(tmp_path / "dump"))
    assert sorted(os.listdir(tmp_path / "dump")) == sorted(k + ".npy" for k in o1)
    assert np.array_equal(np.load(tmp_path / "dump" / "Gu.npy"), o1["Gu"])
    try:
        b.write_outputs({"x": np.zeros(17 << 20, np.float32)}, str(tmp_path / "too_big"))
        raise AssertionError("write_outputs wrote more than 64 MB")
    except RuntimeError:
        assert not os.path.exists(tmp_path / "too_big" / "x.npy")
