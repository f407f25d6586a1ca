"""bench.py's command line without a GPU: a plain run leaves every leg beside the headline off, --full turns each on at its
default, a leg's own option is honoured either way, and --dump-outputs writes the last step's records as float64 .npy files."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(argv):
    sys.path.insert(0, ROOT)
    import bench
    saved = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench, bench.parse()
    finally:
        sys.argv = saved


def test_plain_run_leaves_the_legs_off():
    bench, args = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert args.steps == 7 and args.warmup == 3 and not args.full and args.dump_outputs == ""
    for k in bench.FULL_LEGS:
        assert getattr(args, k) == 0, k


def test_full_turns_every_leg_on_at_its_default():
    bench, args = _parse(["--steps", "7", "--full"])
    assert args.steps == 7 and args.full
    for k, v in bench.FULL_LEGS.items():
        assert getattr(args, k) == v, k
    assert args.cpu_sample > 0 and args.setup_parity == 1 and args.e2e_snps > 0 and args.c4_leg == 1


def test_a_leg_given_explicitly_runs_either_way():
    for extra in ([], ["--full"]):
        _, args = _parse(["--complete-steps", "6", "--cpu-sample", "0"] + extra)
        assert args.complete_steps == 6 and args.cpu_sample == 0


def test_dump_outputs_writes_every_field(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    names = ("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score", "logl_H1")
    res = np.random.default_rng(0).standard_normal((300, 8))
    bench.dump_outputs(str(tmp_path / "out"), np, res, names, 5)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in names)
    for j, k in enumerate(names):
        a = np.load(tmp_path / "out" / (k + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, res[:, j])


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    names = ("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score", "logl_H1")
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 9 * 50)  # room for 50 SNPs of 8 fields + their index
    res = np.random.default_rng(1).standard_normal((300, 8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), np, res, names, 5)
    idx = np.load(tmp_path / "a" / "snp_index.npy")
    assert idx.dtype == np.float64 and idx.size == 50 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "snp_index.npy"))  # the same sample from the same seed
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 8 * 9 * 50 + 10 * 128  # the arrays within the cap, plus one .npy header per file
    for j, k in enumerate(names):
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), res[idx.astype(np.int64), j])
