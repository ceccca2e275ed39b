"""bench.py itself, on a GPU: the one-GPU `--full` line carries the objects the contract asks for and verifies what it times, a
plain run gives the same records with the headline alone, and the N > 1 logic (shards, double-buffered gathers, the hash of
the gathered list) gives the same result list as N = 1 -- run with two ranks sharing the one GPU through the developer backend
(RCCL refuses two ranks on one device, so the gather goes through gloo and host memory there; the RCCL gather itself is
covered by test_packed_shards_and_rccl_gather_single_rank)."""
import json
import os
import socket
import subprocess
import sys

import pytest

from ctag_testlib import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _line(out):
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def test_one_gpu_line_and_two_rank_hash(tmp_path):
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--frames", "192", "--host-frames", "0",
            "--pose-frames", "0", "--latency-calls", "0"]
    dump = str(tmp_path / "out")
    p = subprocess.run(base + ["--full", "--cpu-frames", "24", "--cpu-frames-per-thread", "2", "--dump-outputs", dump], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    one = _line(p.stdout)
    assert one["n_gpus"] == 1 and one["unit"] == "frames/s" and one["frames_ok"] == 192
    assert one["steps"] == 2 and one["ms_per_step"] > 0
    # --dump-outputs: the records of the last timed step, every frame of them (192 frames fit the 64 MB budget)
    assert one["dumped_outputs"]["frames"] == 192
    assert (np.load(os.path.join(dump, "frame_index.npy")) == np.arange(192)).all()
    assert int((np.load(os.path.join(dump, "status.npy")) == 0).sum()) == one["frames_ok"]
    assert int(np.load(os.path.join(dump, "n_markers.npy")).sum()) == one["markers_decoded_last_step"]
    assert np.load(os.path.join(dump, "features_corners.npy")).shape == (192, 100, 16)
    assert one["parity"]["mismatches"] == 0 and one["parity"]["frames_checked"] >= 24
    assert one["roofline"]["bound"] == "hbm" and 0.0 < one["roofline"]["frac"] < 1.0 and one["roofline"]["traffic_source"]
    assert one["cpu_baseline"]["kind"] == "port" and one["cpu_baseline"]["cores"] == 1 and one["cpu_baseline"]["value"] > 0
    assert set(one["issue_roofline"]["kernels"]) >= {"k_edge_refine", "k_welsch", "k_quad_edges_packed"}
    # a plain run (no --full) times the same steps and prints the headline and what they produced, nothing measured beyond them
    plain_dump = str(tmp_path / "plain")
    p = subprocess.run(base + ["--dump-outputs", plain_dump], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    plain = _line(p.stdout)
    assert plain["metric"] == one["metric"] and plain["unit"] == "frames/s" and plain["higher_is_better"] is True and plain["dtype"] == "u8"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["results_sha256"] == one["results_sha256"] and plain["frames_ok"] == 192 and plain["dumped_outputs"]["frames"] == 192
    assert not {"roofline", "issue_roofline", "stage_ms_per_step", "cpu_baseline", "parity", "one_stream", "pose_side"} & set(plain)
    for f in os.listdir(dump):
        assert np.load(os.path.join(plain_dump, f)).tobytes() == np.load(os.path.join(dump, f)).tobytes(), f
    # N = 2 the way the driver starts it: `python bench.py --gpus 2 ...`, no launcher around it -- bench.py starts torch.distributed.run
    # itself as a child process before anything touches the GPU (launch_ranks) and hands back the launcher's exit code
    env = dict(os.environ, CTAG_BENCH_BACKEND="gloo")
    p = subprocess.run(base + ["--gpus", "2", "--cpu-frames", "0"], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    two = _line(p.stdout)
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["frames_per_gpu"] == 96 and two["frames_ok"] == 192
    assert two["results_sha256"] == one["results_sha256"]  # the gathered list equals the one-GPU list
    assert two["config"]["pipelining"].startswith("steps alternate between 2 handles")
    assert "gather_ms" not in two and "rank_stage_ms" not in two  # measured beyond the timed steps: --full only
    # ... and under an explicit launcher (the other command shape of the contract)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + base[1:] + ["--gpus", "2", "--cpu-frames", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _line(p.stdout)["results_sha256"] == one["results_sha256"]


def test_a_rank_that_dies_ends_the_job_non_zero():
    """A rank that fails must end the whole job with a non-zero exit code, promptly: rank 1 is made to leave after the warm-up
    (CTAG_BENCH_FAULT=rank1_exit, a test hook), the launcher ends rank 0 and `python bench.py --gpus 2` returns non-zero."""
    import time
    env = dict(os.environ, CTAG_BENCH_BACKEND="gloo", CTAG_BENCH_FAULT="rank1_exit")
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "64", "--cpu-frames", "0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode != 0 and time.perf_counter() - t0 < 300
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]  # no line from a job that lost a rank


def _ranks_give_the_one_gpu_list(frames, world):
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--frames", str(frames), "--host-frames", "0",
            "--pose-frames", "0", "--latency-calls", "0", "--cpu-frames", "0", "--pipelined-steps", "0"]
    p = subprocess.run(base, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    one = _line(p.stdout)
    assert one["frames_ok"] == frames and one["results_of"].startswith("the last TIMED step") and "the same" in one["results_of"]
    env = dict(os.environ, CTAG_BENCH_BACKEND="gloo", OMP_NUM_THREADS="1")
    p = subprocess.run(base + ["--gpus", str(world)], capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    many = _line(p.stdout)
    per_gpu = (frames + world - 1) // world
    assert many["n_gpus"] == world and many["scaling"] == "strong" and many["frames_ok"] == frames
    assert many["config"]["frames_per_step"] == frames and many["config"]["frames_per_gpu"] == per_gpu
    assert many["results_sha256"] == one["results_sha256"]
    assert many["roofline"]["bound"] == "hbm" and many["roofline"]["frac"] > 0 and many["roofline"]["frames_per_launch"] == per_gpu
    assert many["gather_ms"] is not None and many["gather_ms"] > 0
    assert len(many["rank_stage_ms"]) == world and all(r["edge_refine"] > 0 and r["decimate"] > 0 for r in many["rank_stage_ms"])
    assert "ctag_pack_results" in many["config"]["gather"]  # on RCCL: "ctag_gather (C ABI -> ncclAllGather of packed shards)"
    gb = many["config"]["gather_bytes"]
    assert 0 < gb["packed_local"] <= gb["padded_per_rank"] < gb["fixed_records_per_rank"]


@pytest.mark.parametrize("frames", [256, 250])
def test_eight_ranks_give_the_one_gpu_list(frames):
    """BASELINE config 4's shape before it meets eight GPUs: `python bench.py --gpus 8` (self-launched, eight ranks through the developer
    backend) on 256 frames and on 250 (uneven shards: two ranks own 32 frames, six 31).  Rank 0's gathered list must hash like the
    one-GPU list of the same frames, and the line must carry what a SCALE record is read for: `roofline`, `gather_ms`, every rank's
    per-kernel times and the gather in use.  What the developer backend replaces is the two ncclAllGather calls only: shards are packed
    by ctag_pack_results and unpacked by ctag_gather_end's kernels.
    Needs one GPU per rank: eight ranks on one GPU would keep it open from nine processes at once (the ranks and this one), more
    than a shared GPU box allows.  One-GPU boxes skip it and run test_four_ranks_on_one_gpu_give_the_one_gpu_list instead."""
    import torch
    if torch.cuda.device_count() < 8:
        pytest.skip("needs 8 GPUs (one per rank), found %d" % torch.cuda.device_count())
    _ranks_give_the_one_gpu_list(frames, 8)


def test_four_ranks_on_one_gpu_give_the_one_gpu_list():
    """The same checks with `--gpus 4`, the four ranks sharing this box's one GPU, on 250 frames (uneven shards: 63, 63, 62, 62)."""
    _ranks_give_the_one_gpu_list(250, 4)
