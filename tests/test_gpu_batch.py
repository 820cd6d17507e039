"""Multi-GPU path on the GPU tier, run with one rank (the only size a 1-GPU box offers): the C++ batch driver end to end
(compute -> RCCL gather into rank 0 -> checksum of every gathered strip against its producer's) and the pf_dist_* ABI."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu


def test_pano_batch_one_gpu_three_pairs():
    exe = os.path.join(PKG, "tools", "pano_batch")
    r = subprocess.run([exe, "-pairs", "3", "-size", "640x480", "-flow_alg", "pixflow_search_20", "-gpus", "1", "-verify", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["gpus"] == 1 and res["pairs"] == 3 and res["verified_pairs"] == 3 and res["Mpix/s"] > 0


def test_pano_batch_in_flight_matches_one_at_a_time():
    """-in_flight K: a GPU solves K of its pairs through one set of launches per round and gathers them as one block; with a ragged
    last round.  The gathered strips verify against their producers' checksums, like the one-pair-per-round run."""
    exe = os.path.join(PKG, "tools", "pano_batch")
    out = {}
    for k in ("1", "3"):
        r = subprocess.run([exe, "-pairs", "5", "-size", "640x480", "-flow_alg", "pixflow_low", "-gpus", "1", "-verify", "1", "-in_flight", k], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[k] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert out[k]["pairs"] == 5 and out[k]["verified_pairs"] == 5 and out[k]["in_flight_per_gpu"] == int(k)


def test_pf_dist_self_gather_and_max(pf):
    c = pf.Context(0)
    d = pf.Dist(0, pf.dist_unique_id(), 0, 1)
    n = 1 << 20
    src = np.random.default_rng(3).integers(0, 255, n, dtype=np.uint8)
    a = c.dev_alloc(n); b = c.dev_alloc(n)
    c.upload(a, src)
    d.gather_async(a, b, n)
    d.wait()
    got = c.download(np.empty(n, np.uint8), b)
    assert np.array_equal(got, src)
    assert d.max(3.5) == 3.5
    d.barrier()
    d.close(); c.dev_free(a); c.dev_free(b); c.close()


def test_pano_batch_golden_self_validation(tmp_path):
    """pano_batch -golden: the C++ driver reads the fixture's inputs (exported by tests/golden/export_dense_inputs.py, generated on this
    GPU: synth.py gives the host's bytes on any device), and after the clock requires every strip to be the ORACLE's (SHA-256 from
    tests/golden/dense_9000x4000.sha256.txt) -- what makes a multi-GPU run of config 5 trustworthy without Python."""
    import sys
    from conftest import ROOT
    d = str(tmp_path / "golden_in")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "export_dense_inputs.py"), d, "2"], check=True, timeout=600)
    exe = os.path.join(PKG, "tools", "pano_batch")
    r = subprocess.run([exe, "-pairs", "2", "-size", "9000x4000", "-flow_alg", "pixflow_low", "-gpus", "1", "-golden", d], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["pairs"] == 2 and res["verified_pairs"] == 2 and res["golden_pairs_ok"] == 2
    # a wrong input file is refused, not silently benchmarked
    with open(os.path.join(d, "pair_1235_R.bgra"), "r+b") as f:
        f.seek(12345); f.write(b"\x07")
    r = subprocess.run([exe, "-pairs", "2", "-size", "9000x4000", "-flow_alg", "pixflow_low", "-gpus", "1", "-golden", d], capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "not the fixture's inputs" in r.stderr


def test_bench_forced_dist_path_validates_itself():
    """PANOFLOW_FORCE_DIST=1 on one GPU takes bench.py's multi-rank path (RCCL self-gather inside libpanoflow.so, all-reduced fixture
    verdict): same keys as the single-rank line, fixture_ok true, the gathered slot equal to the oracle fixture's strip."""
    import sys
    from conftest import ROOT
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    lines = {}
    for force in ("0", "1"):
        e = dict(env, PANOFLOW_FORCE_DIST=force)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--no-extras", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=e)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines[force] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    a, b = lines["0"], lines["1"]
    assert set(a) == set(b), set(a) ^ set(b)
    assert a["fixture_ok"] is True and b["fixture_ok"] is True
    assert "pf_dist_" in b["config"]["final_gather"] and "every rank's slot equals its oracle fixture's strip: True" in b["config"]["final_gather"]
    assert b["value"] > 0.8 * a["value"]
    # config 5 read as STRONG scaling (round-4 review, next #5): the eight fixture pairs as one batch, every pair's flows + strip held to its
    # oracle fixture; with the forced RCCL path additionally gathered (8 rounds of one rank) and every gathered strip checked by SHA-256
    for ln in (a, b):
        st = ln["config5_strong"]
        assert st["scaling"] == "strong" and st["pairs_total"] == 8 and st["in_flight_per_rank"] == 8 and st["fixture_ok"] is True and st["value"] > 0
    assert a["config5_strong"]["gathered_strips_equal_fixtures"] is None and b["config5_strong"]["gathered_strips_equal_fixtures"] is True


def test_bench_plain_run_dumps_the_timed_outputs(orc, synth, pf, tmp_path):
    """A plain bench run times exactly --steps steps and prints the headline keys only; --dump-outputs writes what its last timed step
    computed (every pixel at this size) as float32, equal to the oracle's flows and blended strip for the same seeded pair."""
    import sys
    from conftest import ROOT
    cols, rows = 320, 256
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--cols", str(cols), "--rows", str(rows),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0 and res["dtype"] == "f32"
    assert not {"fixture_ok", "roofline", "kernels_ms_per_step", "config5_strong", "cpu_baseline"} & set(res)
    got = {n: np.load(d / (n + ".npy")) for n in ("flow_l2r", "flow_r2l", "novel_view")}
    assert sorted(os.listdir(d)) == ["flow_l2r.npy", "flow_r2l.npy", "novel_view.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    L, R, blend = synth.make_pair_np(cols, rows, 1234)
    r0, r1 = orc.flow_bidir(L, R, pf.max_percentage_by_name("pixflow_low"))
    rout = orc.combine_novel_views(L, R, r0, r1, blend)
    assert np.array_equal(got["flow_l2r"], r0.reshape(-1, 2)) and np.array_equal(got["flow_r2l"], r1.reshape(-1, 2))
    assert np.array_equal(got["novel_view"], rout.reshape(-1, 4).astype(np.float32))
