"""The N > 1 data-parallel path on ONE GPU box: two ranks share cuda:0 and exchange through gloo (RCCL refuses two ranks on one
device), everything else -- rank spawn by bench.py itself, parameter broadcast, per-rank dropout seeds, gradients written
straight into the flat buffer, bucketed all-reduce launched from inside backward on a communication stream, clip + Adam --
is the code the 8-GPU RCCL run executes (the process-group backend is the only difference)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("extra", [[], ["--dtype", "bf16"], ["--dtype", "bf16", "--grad-wire", "bf16"]],
                         ids=["fp32", "bf16mode", "bf16mode_bf16wire"])
def test_bench_launches_its_own_ranks(extra):
    """`python bench.py --gpus 2` with no launcher in the environment must spawn 2 ranks and print ONE JSON line -- for the
    contract's fp32 workload and for BASELINE configs[2] as a mode (bf16 arithmetic / storage / all-reduce payload)."""
    env = dict(os.environ, TAG_DIST_BACKEND="gloo", TAG_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "8", "--full", "--no-cpu-baseline", "--no-alt"] + extra, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_observed"] == 2 and out["config"]["global_batch"] == 16
    assert out["value"] > 0 and out["scaling"] == "weak" and out["comm"]["overlap"] is True
    assert len(out["comm"]["buckets_MB"]) >= 3
    # the self-diagnosing fields of the comm block (round 3): per-bucket durations / exposed time (events exist only on the
    # RCCL path: None under gloo) and the collectives timed alone for both payload types
    comm = out["comm"]
    assert {"bucket_ms_in_step", "exposed_ms_per_step", "comm_only", "payload"} <= set(comm)
    assert comm["payload"] == ("bf16" if "--grad-wire" in extra else "fp32")      # fp32 wire by default, also in the bf16 mode
    for kind in ("fp32", "bf16"):
        leg = comm["comm_only"][kind]
        assert leg["ms_per_step"] > 0 and len(leg["bucket_ms"]) == len(comm["buckets_MB"]) and leg["payload_MB"] > 0
    assert abs(comm["comm_only"]["fp32"]["payload_MB"] - 2 * comm["comm_only"]["bf16"]["payload_MB"]) < 0.1


def test_bench_eight_ranks_on_one_gpu():
    """First contact with 8 ranks, as far as one GPU allows: `python bench.py --gpus 8 --batch 4` (BASELINE configs[2]'s mode)
    self-launches 8 processes that all bind cuda:0 (TAG_SHARE_GPU) and exchange through gloo -- launcher, rank -> device mapping,
    parameter broadcast to 8 replicas, 8 hosts enqueueing the cooperative GRU kernels and the side-stream wgrads into one device,
    bucketed exchange from inside backward, the comm block of the JSON line."""
    env = dict(os.environ, TAG_DIST_BACKEND="gloo", TAG_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
                        "--batch", "4", "--full", "--no-cpu-baseline", "--no-alt", "--dtype", "bf16"], env=env, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["ranks_observed"] == 8 and out["config"]["global_batch"] == 32
    assert out["config"]["parallelism"] == "dp8" and out["scaling"] == "weak" and out["value"] > 0
    comm = out["comm"]
    assert comm["payload"] == "fp32" and comm["overlap"] is True and len(comm["buckets_MB"]) >= 3
    for kind in ("fp32", "bf16"):
        leg = comm["comm_only"][kind]
        assert leg["ms_per_step"] > 0 and len(leg["bucket_ms"]) == len(comm["buckets_MB"])
    import math
    assert math.isfinite(out["loss"])


def test_bench_comm_only_leg():
    """`python bench.py --gpus 2 --comm-only` times nothing but the gradient buckets' all-reduces and prints one JSON line."""
    env = dict(os.environ, TAG_DIST_BACKEND="gloo", TAG_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--comm-only"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and set(out["comm_only"]) == {"fp32", "bf16"} and len(out["buckets_MB"]) >= 3


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import tag_oracle as O
        from tests.test_gpu_path import build_hip_model
        from texttoaudiogrounding_amd import ops
        from texttoaudiogrounding_amd.runner import StrongRunner
        dev = torch.device("cuda:0")
        st = O.init_state(seed=1 + rank, logit_gain=40.0)            # different start per rank: the broadcast must fix it
        model = build_hip_model(st, "dot", dev).train()
        runner = StrongRunner(model, device=str(dev), bucket_bytes=4 << 20)
        batch = O.synthetic_batch(3, 64000, seed=20 + rank, ragged=True)
        fresh = lambda: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        # local gradient of this rank alone (buckets off), then the same step with the overlapped exchange
        torch.manual_seed(7)
        bk, runner.buckets = runner.buckets, None
        runner.forward_backward(fresh())
        local = runner.flat.grad.clone()
        runner.buckets = bk
        torch.manual_seed(7)
        loss = runner.forward_backward(fresh())
        torch.cuda.synchronize()
        assert all(bk.launched)
        both = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(both, local)
        want = both[0] + both[1]
        assert torch.equal(runner.flat.grad, want), (runner.flat.grad - want).abs().max().item()
        assert (both[0] - both[1]).abs().max().item() > 0               # the shards really differ
        p0 = runner.flat.flat.clone()
        runner.optimizer_step()
        runner.loss_value(loss)
        ps = [torch.empty_like(p0) for _ in range(world)]
        dist.all_gather(ps, runner.flat.flat)
        assert torch.equal(ps[0], ps[1]) and not torch.equal(ps[0], p0)  # replicas stay identical after clip + Adam
        # per-replica BatchNorm statistics (no SyncBN in the reference): running stats differ across ranks
        rm = model.audio_encoder.conv_block2.bn1.running_mean.clone()
        rms = [torch.empty_like(rm) for _ in range(world)]
        dist.all_gather(rms, rm)
        assert not torch.equal(rms[0], rms[1])
        if rank == 0:
            open(out, "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_two_ranks_overlapped_allreduce_equals_sum_of_local_gradients(tmp_path):
    out = str(tmp_path / "ok")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert open(out).read() == "ok"
