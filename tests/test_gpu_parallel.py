"""-m gpu: the RCCL plumbing of the data-parallel exchange on ONE GPU (world_size 1): the torch view aliases the
library's gradient buffer (zero copy), all_reduce runs on it in place and the update consumes what it left.
Runs in a fresh interpreter because torch has to be imported before libeesen_hip.so (one shared HIP runtime)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_grad_view_is_zero_copy_and_allreduce_in_place(gpu):
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rccl_plumbing_check.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_PLUMBING_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bench_runs_under_torchrun_with_one_rank(gpu):
    """The driver's multi-GPU launch line with N = 1 (same code path as N > 1 minus the collective)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--T", "100",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0 and '"metric"' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _bench(args, env_extra, timeout=900):
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "EESEN_RCCL_LIBRARY", "EESEN_PERSISTENT", "EESEN_GPU_SHARE", "EESEN_COMM_DEFER"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def test_plain_bench_run_is_the_headline_only_and_dumps_its_last_step(gpu, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W`: the K timed steps and the line, none of the legs --full adds; with
    --dump-outputs DIR the last timed step's outputs as float32 / float64 .npy files, 64 MB at most."""
    import numpy as np
    from eesen_amd import synth
    d, _ = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--T", "100", "--dump-outputs", str(tmp_path)], {})
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["dtype"] == "f32" and d["value"] == pytest.approx(d["config"]["padded_frames_per_step"] * 1e3 / d["ms_per_step"], rel=1e-6)
    assert "cpu_baseline" not in d and "frontend" not in d and "secondary" not in d["config"] and "legs_ms" not in d
    assert d["config"]["f32_mfma_gemm_only"] is None and d["config"]["device_resident_ms_per_step"] is None
    files = {f.name: np.load(f) for f in tmp_path.iterdir()}
    assert set(files) == {"posteriors.npy", "ctc_diff.npy", "params.npy", "grads.npy", "ctc_stats.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
    cfg = synth.config("cfg2")
    batch = synth.make_batch(**{**cfg, "T": 100, "seed": 777})
    post = files["posteriors.npy"]
    assert post.shape == (100 * 32, cfg["K"]) == files["ctc_diff.npy"].shape
    real = np.array([t < batch.lens[s] for t in range(100) for s in range(32)])
    assert np.allclose(post[real].sum(1), 1.0, atol=1e-4)           # softmax rows of the real frames
    assert files["params.npy"].shape == files["grads.npy"].shape == (1 << 20,) and np.all(np.isfinite(files["grads.npy"]))
    assert files["ctc_stats.npy"][1] > 0 and files["ctc_stats.npy"][1] % 32 == 0


def test_bench_secondary_leg_runs_as_a_process_of_its_own(gpu):
    """`bench.py --leg NAME` (round 6): what the default bench run starts once per leg of config.secondary -- a Net's step time depends on
    its process's allocation history, so every leg gets a fresh process.  One JSON record on stdout, every layer pass persistent."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--leg", "wsj_recipe_shape_S10"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert 5.0 < d["ms_per_minibatch"] < 100.0 and d["recoveries"] == 0
    assert d["persistent_layer_passes"]["fwd"] == d["persistent_layer_passes"]["bwd"] == d["persistent_layer_passes"]["of"] > 0


def test_bench_line_describes_the_real_rccl_at_world_size_one(gpu):
    """The self-describing N > 1 line with the REAL librccl, at the only world size a one-GPU box offers:
    `config.comm` names the library the linker resolved (not the stand-in), its version, the one rank RCCL itself counts, the
    device's PCI bus id; n_gpus = distinct devices = 1; the rank-consistency check ran."""
    d, _ = _bench(["--gpus", "1", "--force-dist", "--steps", "2", "--warmup", "1", "--main-only", "--T", "120"], {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29547"})
    c = d["config"]["comm"]
    assert c["stand_in"] is False and "librccl" in c["library"] and c["rccl_version"] >= 20000, c
    assert c["world"] == 1 and c["world_seen"] == 1 and c["rank_seen"] == 0 and c["device_seen"] == c["device"] == 0, c
    assert c["distinct_devices"] == 1 and c["ranks_share_devices"] is False and len(c["devices"]) == 1 and ":" in c["devices"][0]
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 1 and d["config"]["ranks_bit_identical"] is True
    assert d["config"]["comm_stand_in"] is False and d["config"]["gradient_exchange"].startswith("RCCL ")
    # a full-width cfg2 net, persistent kernels: the schedule is the deferred one, chosen from the backward plan (164 registers: 176 free < 256)
    assert d["config"]["exchange_schedule"].startswith("deferred") and d["config"]["exchange_rule"].startswith("auto")
    k = d["config"]["kernels"]
    assert k["backward"] == ["lstm_bwd_persistent_q4_kernel<8,4>"] and k["backward_tile"]["free_vgprs_per_simd_lane"] < 256, k


def test_bench_with_eight_ranks_on_one_gpu_through_the_rccl_shaped_stand_in(gpu):
    """8-GPU pre-flight: `bench.py --gpus 8` -- self-launch of eight ranks, rendezvous, buckets, closing
    barrier, rank 0's JSON -- with every rank holding PERSISTENT grids on the one GPU (each process sizes its grids against 32 CUs:
    the share the communicator works out itself; 2 x BiLSTM of 64 cells, S = 16: 8 x (16 + 16) workgroups co-resident) and the stand-in's all-reduce
    kernels in RCCL's footprint (FAKE_RCCL_SHAPE=rccl: 256 VGPRs x 512 threads, 37.7 KB LDS).  The line must say what it is:
    eight ranks, ONE device, a stand-in -- and that the eight models are still identical after the steps."""
    from tests.test_gpu_multirank import fake_rccl_path
    d, err = _bench(["--gpus", "8", "--steps", "3", "--warmup", "1", "--main-only", "--T", "100", "--H", "64", "--S", "16", "--layers", "2"],
                    dict(EESEN_RCCL_LIBRARY=fake_rccl_path(), FAKE_RCCL_QUIET="1", FAKE_RCCL_SHAPE="rccl", FAKE_RCCL_BLOCKS="4", EESEN_BENCH_SHARE_GPU="0"), timeout=1200)
    # (FAKE_RCCL_BLOCKS=4: 8 ranks x 4 = the 32 workgroups of ONE RCCL kernel on the device, each with a whole CU's registers.  No
    # EESEN_GPU_SHARE: the communicator finds its eight ranks on one device and sizes every process against 1/8 of it -- VERDICT r5 item 8)
    assert "8 of the 8 data-parallel ranks share this rank's device: persistent grids are sized against 1/8" in err, err[-3000:]
    c = d["config"]
    assert d["n_gpus"] == 1 and c["ranks"] == 8 and c["parallelism"] == "dp8" and c["global_batch_utterances"] == 8 * 16
    assert c["ranks_share_devices"] is True and c["distinct_devices"] == 1 and c["comm_stand_in"] is True and c["comm_world_seen"] == 8
    assert len(c["comm"]["devices"]) == 8 and len(set(c["comm"]["devices"])) == 1 and "libfake_rccl" in c["comm"]["library"]
    assert c["gradient_exchange"].startswith("TEST STAND-IN")
    assert c["ranks_bit_identical"] is True
    assert c["padded_frames_per_step"] == 8 * 16 * 100
    # every rank's layer passes ran on the persistent kernels (rank 0 reports; a rank that failed its probing step makes ALL fall back)
    assert c["kernels"]["backward"] == ["lstm_bwd_persistent_q4_kernel<2,4>"] and c["kernels"]["forward"][0].startswith("lstm_fwd_persistent"), c["kernels"]
    # 64 cells: the 4 x 32 tile leaves >= 256 registers per SIMD lane -- the one class of shapes whose buckets stay overlapped
    assert c["exchange_schedule"].startswith("overlapped")
    ex = d["roofline"]["exchange"]
    assert [b["layer"] for b in ex["buckets"]] == [2, 1, 0] and all(b["ms"] > 0 for b in ex["buckets"])
    assert "persistent path failed" not in err, err[-3000:]


def test_bench_with_two_ranks_on_one_gpu_through_the_stand_in(gpu):
    """bench.py's world > 1 path itself -- self-launch, TCP rendezvous, the library's communicator attached to the Net, the
    barrier's all-reduce of dt / padded / real frames over the ranks, rank 0's one JSON line with the exchange report -- executed
    with TWO ranks before an 8-GPU node ever sees it.  Both ranks share GPU 0 (EESEN_BENCH_SHARE_GPU), the
    collective is the test-only stand-in for librccl.so (tests/native/fake_rccl.hip), and two processes cannot both hold a
    persistent recurrence grid on one GPU, so the per-step kernels run: this is plumbing, never a measurement."""
    import json
    from tests.test_gpu_multirank import fake_rccl_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EESEN_RCCL_LIBRARY=fake_rccl_path(), EESEN_PERSISTENT="0", FAKE_RCCL_QUIET="1", EESEN_BENCH_SHARE_GPU="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--main-only", "--T", "120"],
                       capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    # two ranks on ONE device through the stand-in: the line says so itself -- n_gpus counts distinct devices
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 2 and d["config"]["ranks_share_devices"] is True and d["config"]["comm_stand_in"] is True
    assert d["config"]["comm"]["world_seen"] == 2 and d["config"]["comm"]["distinct_devices"] == 1 and d["config"]["ranks_bit_identical"] is True
    assert d["config"]["gradient_exchange"].startswith("TEST STAND-IN") and d["config"]["exchange_schedule"].startswith("overlapped")   # per-step kernels: nothing to defer behind
    assert d["config"]["global_batch_utterances"] == 64 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["padded_frames_per_step"] == 2 * 32 * 120           # the ranks' frames were summed over the communicator
    assert d["value"] == pytest.approx(d["config"]["padded_frames_per_step"] * 1e3 / d["ms_per_step"], rel=1e-6)
    ex = d["roofline"]["exchange"]
    assert ex["bound"] == "xgmi" and ex["peak"] == pytest.approx(7 * 153.0)
    assert len(ex["buckets"]) == 5 and [b["layer"] for b in ex["buckets"]] == [4, 3, 2, 1, 0]     # affine, then the LSTM layers top-down
    assert abs(sum(b["MB"] for b in ex["buckets"]) - 84.8) < 0.2                                   # 84.8 MB at cfg2
    assert all(b["ms"] > 0 for b in ex["buckets"]) and ex["ms_per_step"] > 0 and ex["exposed_ms_per_step"] >= 0
    assert d["phase_ms_per_step"]["allreduce"] == pytest.approx(ex["ms_per_step"]) and "allreduce_exposed" in d["phase_ms_per_step"]


def test_bench_check_full_cfg3_with_eight_ranks_through_the_stand_in(gpu):
    """`bench.py --gpus 8 --check full_cfg3` -- what the driver's 8-GPU box can run to hold the REAL exchange against the reference:
    rank r takes shard r of BASELINE configs[2]'s global minibatch (256 utterances, T = 1000, 4 x 512), the communicator sums the
    gradients, and the sum is compared with tests/golden/full_cfg3.npz (one reference process at --num-sequence 256) at the
    fixture's bars.  Here: eight ranks on the one GPU through the stand-in, per-step kernels (eight 256-workgroup persistent grids
    cannot share a device), so that the check's own control flow and arithmetic have run before the first 8-GPU box sees them."""
    from tests.test_gpu_multirank import fake_rccl_path
    d, err = _bench(["--gpus", "8", "--steps", "1", "--warmup", "0", "--main-only", "--T", "100", "--check", "full_cfg3"],
                    dict(EESEN_RCCL_LIBRARY=fake_rccl_path(), FAKE_RCCL_QUIET="1", EESEN_BENCH_SHARE_GPU="0", EESEN_PERSISTENT="0"), timeout=1800)
    c = d["config"]["check_full_cfg3"]
    assert c.get("ok") is True, c
    assert d["config"]["check_full_cfg3_ok"] is True
    assert c["shards"] == 8 and c["utterances_per_shard"] == 32 and c["every_rank_sees_the_same_sum"] is True and c["tensors"] == 50
    assert c["ln_p_worst_rel_err_per_sequence"] < 1e-4 and c["worst_error_over_its_bar"] < 1.0, c
    assert d["config"]["ranks"] == 8 and d["config"]["ranks_bit_identical"] is True and d["config"]["comm_stand_in"] is True
