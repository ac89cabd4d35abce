"""bench.py's multi-GPU branch on a real GPU at world 1: launched by torch.distributed.run with
one rank, it creates the RCCL process group (backend "nccl"), all-reduces the verification
counters and the step time over RCCL, and runs hcdist.gather_encoded (hc_pack_batch on the GPU,
the RCCL all-gather of the encoded sizes) with --gather: the path the driver's N-GPU runs take,
minus the point-to-point sends that need a second GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_plain_run_dumps_its_outputs(gpu, oracle_mod, tmp_path):
    """a plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line alone (nothing
    that needs --full), and --dump-outputs leaves the last step's outputs as float .npy files:
    every stream coded with status 0 and its full length back, the sampled streams' decoded bytes
    equal to the synthetic inputs and their encoded bytes to the oracle's encodings"""
    import numpy as np
    S, N = 24, 512 * 512
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(S), "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["bit_exact"] is True
    assert (r["unit"], r["higher_is_better"], r["dtype"], r["n_gpus"]) == ("GiB/s", True, "u8", 1)
    assert not {"cpu_baseline", "configs", "weak_scaling"} & set(r) and "measured_copy_GBps" not in r["roofline"]
    d = {f.name[:-4]: np.load(f) for f in tmp_path.iterdir()}
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64_000_000
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["encode_status"].tolist() == [0] * S == d["decode_status"].tolist()
    assert d["decoded_len"].tolist() == [N] * S
    picked = d["sample_streams"].astype(int).tolist()
    assert len(picked) == 16 and picked == sorted(set(picked)) and picked[-1] < S
    raws = [oracle_mod.synth("photo", k).tobytes() for k in picked]
    assert d["decoded_sample"].astype(np.uint8).tobytes() == b"".join(raws)
    elens = d["encoded_len"].astype(int)
    assert d["encoded_sample"].size == int(elens[picked].sum())
    at = 0
    w = np.arange(2 * N + 4096) % 251 + 1
    for i, k in enumerate(picked):
        got = d["encoded_sample"][at:at + elens[k]].astype(np.uint8)
        at += elens[k]
        assert d["encoded_checksum"][k] == float((got.astype(np.int64) * w[:got.size]).sum())
        if i < 3:
            st, want = oracle_mod.compress(raws[i], True, False, 512)
            assert st == 0 and got.tobytes() == want, k


def test_bench_world1_rccl(gpu):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--streams", "256", "--steps", "2", "--warmup", "1", "--gather", "--no-configs",
           "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["process_group"] == {"backend": "nccl", "world": 1}
    assert r["bit_exact"] is True and r["value"] > 0 and r["n_gpus"] == 1
    g = r["gather"]
    assert g["rank0_spot_check"] is True and g["bytes_to_rank0"] > 0
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "world1_rccl.log"), "w") as f:
        f.write(lines[0] + "\n")
