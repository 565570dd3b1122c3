"""CPU, 2 ranks (gloo): ``python bench.py --gpus 2`` outside any launcher must start two ranks itself and report
``n_gpus: 2`` (round 1's bench.py parsed --gpus and ignored it).  The per-step work is a stub (--stub-workload: the HIP
path needs a GPU); the launch plumbing - self-spawn under torch.distributed.run, ranks from the environment, barrier,
MAX-over-ranks timing, rank 0 printing ONE JSON line - is the code every real mode of bench.py runs."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, env_extra=None, timeout=240):
    env = dict(os.environ, AUDIOCAPTION_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + argv, env=env, cwd=REPO, timeout=timeout,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # exactly one JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_2_self_spawns_two_ranks():
    res = _run(["--gpus", "2", "--steps", "4", "--warmup", "1", "--stub-workload"])
    assert res["n_gpus"] == 2 and res["steps"] == 4 and res["warmup"] == 1
    assert res["config"]["backend"] == "gloo" and res["config"]["requested_gpus"] == 2
    assert res["scaling"] == "weak" and res["value"] > 0 and res["ms_per_step"] > 0
    # the line says where every rank sat (two different processes, ranks 0 and 1)
    assert [r["rank"] for r in res["ranks"]] == [0, 1] and res["ranks"][0]["pid"] != res["ranks"][1]["pid"]


def test_bench_under_a_launcher_reads_the_ranks_from_the_environment():
    """The driver's own command: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N."""
    env = dict(os.environ, AUDIOCAPTION_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", "29731", os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3",
                        "--warmup", "1", "--stub-workload"], env=env, cwd=REPO, timeout=240, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    assert json.loads(lines[0])["n_gpus"] == 2


def test_bench_gpus_8_stub_describes_every_rank():
    """The driver's 8-GPU command on CPU ranks (gloo): the line carries one record per rank, per-rank seconds and the
    collective timing object, so that the first real 8-GPU run describes itself."""
    res = _run(["--gpus", "8", "--steps", "3", "--warmup", "1", "--stub-workload"], timeout=600)
    assert res["n_gpus"] == 8 and [r["rank"] for r in res["ranks"]] == list(range(8))
    assert len({r["pid"] for r in res["ranks"]}) == 8 and len(res["seconds_per_rank"]) == 8
    assert res["rccl"]["world_size"] == 8 and res["rccl"]["backend"] == "gloo"
    assert res["rccl"]["grad_sync_default"] == "all_reduce"          # rs_ag only on RCCL with >= 4 ranks
    assert res["ms_per_step"] * 1e-3 * res["steps"] >= max(res["seconds_per_rank"]) - 1e-9


def test_default_gradient_sync_by_backend_and_world_size():
    from audiocaption_amd.train import default_grad_sync
    assert default_grad_sync(8, "nccl") == "rs_ag" and default_grad_sync(4, "nccl") == "rs_ag"
    assert default_grad_sync(2, "nccl") == "all_reduce" and default_grad_sync(8, "gloo") == "all_reduce"


def test_bench_single_rank_stub():
    res = _run(["--steps", "2", "--warmup", "0", "--stub-workload"])
    assert res["n_gpus"] == 1


@pytest.mark.gpu
def test_bench_two_ranks_real_workload_on_one_gpu():
    """The N > 1 flow of the REAL inference bench (clips sharded over ranks, no data-path collective, barrier + MAX timing,
    rank records, per-rank seconds) with two gloo ranks sharing the only GPU of the box - RCCL refuses two ranks on one
    device, everything else is the code an 8-GPU run executes."""
    res = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4", "--seconds", "2", "--max-length", "6",
                "--full", "--no-tiers", "--no-train", "--no-effb2", "--no-steady-state", "--no-cpu-baseline"], timeout=600)
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 8 and res["value"] > 0
    assert [r["rank"] for r in res["ranks"]] == [0, 1] and len(res["seconds_per_rank"]) == 2
    assert res["rccl"]["world_size"] == 2 and res["scaling"] == "weak"
    assert abs(res["value"] - 8 * 2 / (res["ms_per_step"] * 2e-3)) < 1e-6 * res["value"]


@pytest.mark.gpu
def test_bench_plain_run_reports_the_headline_only(tmp_path):
    """Without --full the real inference bench times the headline and stops: the line carries what the timed steps
    measured and none of the secondary measurements, and no details file is written."""
    details = tmp_path / "details.json"
    res = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--seconds", "2", "--max-length", "6",
                "--details-file", str(details)], timeout=600)
    assert res["n_gpus"] == 1 and res["steps"] == 2 and res["warmup"] == 1 and res["higher_is_better"] is True
    assert res["unit"] == "clips/s" and res["config"]["global_batch"] == 4
    assert abs(res["value"] - 4 * 2 / (res["ms_per_step"] * 2e-3)) < 1e-6 * res["value"]
    assert not [k for k in res if k.startswith(("value_", "latency_", "train_", "effb2_", "ingest_", "clotho_", "steady_"))]
    assert not {"cpu_baseline", "rccl", "details_file", "logmel_hbm_frac"} & set(res)
    assert "sustained_mfma_tflops_measured" not in res["roofline"] and not details.exists()


def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs: what the last timed step returned, as float32 / float64 .npy files; seeded inputs, so two runs with
    the same arguments write the same arrays."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        res = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--stub-workload", "--dump-outputs", str(d)])
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    assert list(dumps[0]) == ["y.npy"] and dumps[0]["y.npy"].dtype == np.float32
    assert dumps[0]["y.npy"].shape == (128, 128) and np.array_equal(dumps[0]["y.npy"], dumps[1]["y.npy"])


def test_dump_outputs_samples_the_same_rows_of_every_array_within_the_budget(tmp_path):
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    import torch
    steps = torch.tensor([True, True, False])
    arrays = bench.host_outputs({"logit": torch.arange(64 * 3 * 100, dtype=torch.float16).view(64, 3, 100),
                                 "seq": torch.arange(64 * 3).view(64, 3), "attn_emb_len": [5] * 64,
                                 "note": "not an array"}, steps_ran=steps.numpy())
    assert sorted(arrays) == ["attn_emb_len", "logit", "seq"]
    assert arrays["logit"].dtype == np.float32 and arrays["seq"].dtype == np.float64
    assert not arrays["logit"][:, 2].any() and arrays["seq"][3, 1] == 10          # the step that did not run is zeroed
    names = bench.dump_outputs(str(tmp_path), arrays, budget=20_000)
    got = {n: np.load(tmp_path / f"{n}.npy") for n in names}
    assert sum(a.nbytes for a in got.values()) <= 20_000
    rows = got["sample_rows"].astype(np.int64)
    assert 0 < len(rows) < 64 and np.array_equal(got["seq"], arrays["seq"][rows])
    assert np.array_equal(got["logit"], arrays["logit"][rows])
    again = bench.dump_outputs(str(tmp_path / "again"), arrays, budget=20_000)
    assert again == names and np.array_equal(np.load(tmp_path / "again" / "sample_rows.npy"), got["sample_rows"])
