"""What the several-rank tests share.  For a test: ``free_port`` and ``run_ranks`` (one child process per rank, the result of rank 0).
For a worker script (tests/_*ddp_worker.py, started by ``run_ranks`` with RANK / WORLD_SIZE / MASTER_* / TQ_TEST_BACKEND set):
``init_rank`` and ``gather``.  With fewer GPUs than ranks the ranks share cuda:0 and the process group is gloo."""

import json
import os
import socket
import subprocess
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):   # (a worker is started as a script: the package and conftest.py must be importable)
    if _p not in sys.path:
        sys.path.insert(0, _p)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker_script, world=2, extra_env=None, timeout=400, tag="DDP_RESULT"):
    """Run tests/``worker_script`` once per rank (RCCL, backend "nccl", when the box has a GPU per rank, otherwise gloo); every rank must
    exit with status 0.  Returns the dict that rank 0 printed as JSON behind ``tag``."""
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), TQ_TEST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", worker_script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-6000:]}"
    line = [l for l in outs[0].splitlines() if l.startswith(tag + " ")][-1]
    res = json.loads(line[len(tag) + 1:])
    print(backend, res)
    return res


def init_rank():
    """(rank, world, device, backend) of this worker process, its process group initialised"""
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = os.environ.get("TQ_TEST_BACKEND", "gloo")
    dev = torch.device("cuda", rank % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    if backend == "nccl":
        from tqdne_amd.trainer import init_process_group   # (side streams first, then the communicator)
        init_process_group("nccl", device=dev, rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, world, dev, backend


def gather(t):
    """``t`` of every rank, as CPU tensors"""
    t = t.to(torch.device("cuda", torch.cuda.current_device())) if dist.get_backend() == "nccl" else t.cpu()
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [o.cpu() for o in out]
