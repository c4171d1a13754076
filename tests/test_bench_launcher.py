"""`python bench.py --gpus N` must start itself: with WORLD_SIZE unset and --gpus > 1 the script
re-executes under torch.distributed.run, one rank per GPU, and rank 0's JSON line is the last line of stdout.  No GPU
here: LS_BENCH_DRY_RUN makes the ranks rendezvous over gloo and stop before touching a device."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_spawns_its_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["LS_BENCH_DRY_RUN"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line == {"dry_run": True, "n_gpus": 2, "ranks_seen": 2, "steps": 4, "warmup": 1}


def test_bench_config_presets_name_baseline_configs_verbatim():
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        names = json.load(f)["configs"]
    assert [c["name"] for c in bench.BASELINE_CONFIGS] == names


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    """--dump-outputs: output_ids / spec_mask / the last step's tokens / counters of the decode state, float64 and exact."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from types import SimpleNamespace
    import bench
    ids = torch.tensor([[1000, 128255, 7, 9, 11, 0, 0]], dtype=torch.int64)
    st = SimpleNamespace(output_ids=ids, spec_mask=torch.zeros_like(ids), emitted=5, count=2, num=3)
    bench.dump_outputs(str(tmp_path / "out"), st, 2)
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in ("output_ids", "spec_mask", "last_step_tokens", "counters")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["output_ids"], ids.numpy().astype(np.float64))
    assert np.array_equal(got["last_step_tokens"], [[7.0, 9.0, 11.0]])
    assert np.array_equal(got["counters"], [5.0, 2.0, 3.0])


def test_plain_run_and_full_options_parse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
