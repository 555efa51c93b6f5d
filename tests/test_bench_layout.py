"""bench.py's `--gpus N` contract: the line measures N GPUs or the run
refuses. On the CPU: the layout planner with stand-in device counts, and the real script on
a host without a GPU, which must exit 2 with the reason rather than measure one GPU; the
sample that `--dump-outputs` writes, over a stand-in store. On the GPU (`-m gpu`): a plain
run of the real script is lean and dumps the same outputs twice, `--full` adds the rest."""
import os
import pathlib
import subprocess
import sys

import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402


def devices(n):
    calls = []

    def count():
        calls.append(1)
        return n
    count.calls = calls
    return count


def test_single_gpu_needs_no_device_query():
    c = devices(0)
    assert bench.plan_layout(1, {}, c) == {"mode": "single", "world": 1}
    assert not c.calls


def test_in_process_handle_over_n_devices():
    lay = bench.plan_layout(4, {}, devices(8))
    assert lay == {"mode": "in-process", "world": 4, "devices": [0, 1, 2, 3]}


@pytest.mark.parametrize("n", [0, 1, 3])
def test_in_process_refuses_fewer_devices(n):
    with pytest.raises(bench.LayoutError, match=rf"needs 4 HIP devices; {n} visible"):
        bench.plan_layout(4, {"HIP_VISIBLE_DEVICES": "0"}, devices(n))


def test_launcher_world_must_equal_gpus():
    with pytest.raises(bench.LayoutError, match="WORLD_SIZE=2"):
        bench.plan_layout(8, {"WORLD_SIZE": "2", "LOCAL_WORLD_SIZE": "2"}, devices(8))
    with pytest.raises(bench.LayoutError, match="WORLD_SIZE=8"):
        bench.plan_layout(1, {"WORLD_SIZE": "8", "LOCAL_WORLD_SIZE": "8"}, devices(8))


def test_launcher_needs_a_device_per_local_rank():
    env = {"WORLD_SIZE": "8", "LOCAL_WORLD_SIZE": "8"}
    assert bench.plan_layout(8, env, devices(8)) == {"mode": "launcher", "world": 8}
    with pytest.raises(bench.LayoutError, match="8 ranks on this node need 8 HIP devices"):
        bench.plan_layout(8, env, devices(1))
    # the one-GPU test mode (two ranks sharing GPU 0 over the host exchange) asks no device count
    c = devices(1)
    assert bench.plan_layout(2, {"WORLD_SIZE": "2"}, c, same_device=True)["mode"] == "launcher"
    assert not c.calls


def test_multi_shards_diagnostic_is_one_gpu_only():
    with pytest.raises(bench.LayoutError, match="--multi-shards"):
        bench.plan_layout(2, {}, devices(8), multi_shards=2)
    assert bench.plan_layout(1, {}, devices(1), multi_shards=2)["mode"] == "single"


def run_bench(args, env_extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, str(REPO / "bench.py"), *args], cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=300)


def test_script_refuses_gpus_2_without_two_devices():
    """The real script on a host with no visible GPU: exit 2, reason on stderr, no JSON line."""
    r = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], {})
    assert r.returncode == 2, r.stderr[-2000:]
    assert "needs 2 HIP devices" in r.stderr
    assert r.stdout.strip() == ""


def test_script_refuses_launcher_mismatch():
    r = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                  {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2, r.stderr[-2000:]
    assert "WORLD_SIZE=1" in r.stderr
    assert r.stdout.strip() == ""


class _FakeCtx:
    """col_names / col_find / col_download / weights_download over numpy arrays (the calls
    bench.state_digests makes)."""
    def __init__(self, cols, w):
        self.cols, self.w = cols, w

    def col_names(self):
        return list(self.cols)

    def col_find(self, name):
        return name

    def col_download(self, c):
        return self.cols[c]

    def weights_download(self):
        return self.w


def _population(n=12, seed=0):
    import numpy as np
    r = np.random.default_rng(seed)
    return {"x_1": r.standard_normal((2, n)), "v": r.standard_normal((2, n)), "a": r.standard_normal(n)}, \
        r.standard_normal(n)


def test_self_check_digests_and_verdict():
    """a sharded line carries its own parity proof. The digests of a shard
    slice of one population equal those of the same slice held by a shard; the verdict passes
    only when every shard and the evidence agree."""
    cols, w = _population()
    full = _FakeCtx(cols, w)
    shard1 = _FakeCtx({k: v[..., 6:12] for k, v in cols.items()}, w[6:12])
    ref = [bench.state_digests(full, 0, 6), bench.state_digests(full, 6, 12)]
    assert bench.state_digests(shard1, 0, 6) == ref[1]
    assert bench.state_digests(full, 0, 12) != ref[0]
    ok = bench.check_verdict(ref, list(ref), -1.5, -1.5)
    assert ok["exact_vs_1gpu"] and ok["mismatched_shards"] == []
    bench.refuse_on_mismatch(ok)                       # passes silently


def test_self_check_mismatch_refuses_the_line():
    cols, w = _population()
    full = _FakeCtx(cols, w)
    ref = [bench.state_digests(full, 0, 6), bench.state_digests(full, 6, 12)]
    bad_w = w.copy()
    bad_w[8] = -bad_w[8]                               # one weight of shard 1 differs
    got = [ref[0], bench.state_digests(_FakeCtx(cols, bad_w), 6, 12)]
    v = bench.check_verdict(ref, got, -1.5, -1.5)
    assert not v["exact_vs_1gpu"] and v["mismatched_shards"] == [1]
    with pytest.raises(SystemExit) as e:
        bench.refuse_on_mismatch(v)
    assert e.value.code == 2
    v = bench.check_verdict(ref, list(ref), -1.5, -1.5000000000000002)   # the evidence alone
    assert not v["exact_vs_1gpu"] and not v["evidence_equal"]
    with pytest.raises(SystemExit):
        bench.refuse_on_mismatch(v)


class _FakeStore(_FakeCtx):
    """_FakeCtx plus n / col_dim / col_gather_rows: what bench.sample_outputs reads."""
    def __init__(self, cols, w):
        super().__init__(cols, w)
        self.n = len(w)

    def col_dim(self, c):
        return 1 if self.cols[c].ndim == 1 else self.cols[c].shape[0]

    def col_gather_rows(self, c, idx):
        return self.cols[c][..., idx]


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: the same seeded sample of particles every time, every array float64 and
    the rows of the population at the sampled indices, the files within the byte budget."""
    import numpy as np
    cols, w = _population(n=5000, seed=3)
    a = bench.sample_outputs(_FakeStore(cols, w), -12.5)
    b = bench.sample_outputs(_FakeStore(cols, w), -12.5)
    assert sorted(a) == ["col_a", "col_v", "col_x_1", "log_evidence", "log_weights", "sample_index"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == 5000                            # fewer particles than the sample: all of them
    assert np.array_equal(idx, np.arange(5000))
    small = bench.sample_outputs(_FakeStore(cols, w), -12.5, budget=7 * 8 * 100)   # 5 column rows + w + index
    idx = small["sample_index"].astype(np.int64)
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx[-1] < 5000
    assert np.array_equal(small["col_x_1"], cols["x_1"][:, idx])
    assert np.array_equal(small["col_a"], cols["a"][idx])
    assert np.array_equal(small["log_weights"], w[idx])
    assert small["log_evidence"].tolist() == [-12.5]
    nbytes = bench.dump_outputs(tmp_path / "out", small)
    assert nbytes <= 7 * 8 * 100 + 8
    files = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert files == sorted(k + ".npy" for k in small)
    assert np.array_equal(np.load(tmp_path / "out" / "col_v.npy"), small["col_v"])


def _bench_line(args):
    import json
    r = run_bench(["--gpus", "1", "--particles", "20000", "--T", "12", *args], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path, gpu_available):
    """A plain run times its steps and nothing else (no per-kernel pass, no CPU legs); with
    --dump-outputs two runs of the same arguments write the same files, bit for bit."""
    import numpy as np
    args = ["--steps", "3", "--warmup", "1"]
    line = _bench_line([*args, "--dump-outputs", str(tmp_path / "a")])
    _bench_line([*args, "--dump-outputs", str(tmp_path / "b")])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(20000 * 12 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["breakdown_ms_per_run"] is None
    assert line["roofline"]["dominant_kernel"] is None and line["roofline"]["frac"] > 0
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert {"log_weights.npy", "log_evidence.npy", "sample_index.npy", "col_x_1.npy", "col_x_13.npy"} <= set(names)
    total = 0
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert a.dtype == np.float64 and np.array_equal(a, b), nm
        assert np.all(np.isfinite(a)), nm
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "col_x_13.npy").shape == (2, bench.DUMP_PARTICLES)
    assert np.load(tmp_path / "a" / "log_evidence.npy")[0] == line["log_evidence_last"]


@pytest.mark.gpu
def test_full_run_adds_the_kernel_breakdown_and_the_cpu_legs(gpu_available):
    line = _bench_line(["--steps", "2", "--warmup", "1", "--full", "--cpu-particles", "20000", "--cpu-T", "12",
                        "--cpu-1t-particles", "20000"])
    assert line["full"] is True and line["ms_per_step"] > 0
    assert line["breakdown_ms_per_run"]["propagate"] > 0
    assert line["roofline"]["dominant_kernel"]["achieved"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["gpu_over_cpu"] > 0
