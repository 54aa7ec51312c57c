"""bench.py's contract: a plain run times exactly --steps rounds and prints the headline line; --dump-outputs writes what the last timed step
computed, the same for every run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), "stdout must hold the one JSON line and nothing else: " + r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()), {k: a.dtype for k, a in out.items()}
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_score_sample_is_fixed_and_bounded():
    import bench
    assert bench.score_positions(bench.SCORE_SAMPLE) is None
    p = bench.score_positions(100_000_000)
    assert np.array_equal(p, bench.score_positions(100_000_000))
    assert len(p) == bench.SCORE_SAMPLE and p[0] >= 0 and p[-1] < 100_000_000 and np.all(np.diff(p) > 0)
    q = bench.score_positions(bench.SCORE_SAMPLE + 1)
    assert len(q) == bench.SCORE_SAMPLE and q[-1] <= bench.SCORE_SAMPLE and np.all(np.diff(q) > 0)


def test_dump_outputs_writes_floats_within_the_limit(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path / "d"), {"a": np.arange(5, dtype=np.int32), "b": np.ones(3, np.float32)})
    z = _load(str(tmp_path / "d"))
    assert z["a"].dtype == np.float64 and np.array_equal(z["a"], np.arange(5)) and z["b"].dtype == np.float32
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros((64 << 20) // 8 + 1)})
    assert not (tmp_path / "e").exists()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_round(tmp_path):
    """A run without --full: the headline fields, exactly --steps timed rounds, none of what --full adds; the dump is the last round's tree, train
    metric and scores -- bit-identical to the same rounds trained here, and to a second run of the same arguments."""
    from ranklib_amd import _native as N
    from ranklib_amd import synth
    steps, warmup = 3, 1
    args = ["--steps", steps, "--warmup", warmup, "--shape", "c0"]
    o = _bench(*(args + ["--dump-outputs", tmp_path / "a"]))
    assert all(k in o for k in HEADLINE) and o["steps"] == steps and o["warmup"] == warmup
    assert o["ms_per_step"] > 0 and abs(o["value"] * o["ms_per_step"] / 1000.0 - 1.0) < 1e-9
    assert "roofline" not in o and "cpu_baseline" not in o and "sustained_rounds_per_s" not in o["config"]
    a = _load(str(tmp_path / "a"))

    n_docs, n_feat, kind, _, n_leaves = synth.SHAPES["c0"]
    X, lab, qoff, _ = synth.make_shard(n_docs, n_feat, kind, 0, 1)
    g = N.Trainer(n_trees=steps + warmup, n_leaves=n_leaves)
    g.set_train(X, lab, qoff)
    g.init()
    g.boost_rounds_async(steps + warmup)
    g.sync()
    tree = g.get_tree(steps + warmup - 1).trimmed()
    assert set(a) == {"tree_" + k for k in tree} | {"train_metric", "scores"}
    for k, v in tree.items():
        assert np.array_equal(a["tree_" + k], v.astype(a["tree_" + k].dtype)), k
    assert np.array_equal(a["scores"], g.array("SCORE"))
    assert a["train_metric"][0] == g.round_metrics(steps + warmup - 1)[0]
    assert a["train_metric"][0] == np.float32(o["config"]["ndcg10_train_after_%d_rounds" % (steps + warmup)])

    _bench(*(args + ["--dump-outputs", tmp_path / "b"]))
    b = _load(str(tmp_path / "b"))
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_infer_run_dumps_the_scores(tmp_path):
    o = _bench("--workload", "infer", "--docs", 50000, "--trees", 64, "--infer-train-rounds", 8, "--steps", 2, "--warmup", 1, "--dump-outputs", tmp_path)
    assert all(k in o for k in HEADLINE) and o["steps"] == 2 and o["ms_per_step"] > 0 and "cpu_baseline" not in o
    z = _load(str(tmp_path))
    assert set(z) == {"scores"} and z["scores"].shape == (50000,) and z["scores"].dtype == np.float32 and np.all(np.isfinite(z["scores"]))
