"""GPU box, ONE GPU: what can be proven about the multi-GPU and multi-thread paths without a second device.

  * ``bench.py`` and the BASELINE config-4 example under ``torch.distributed.run --nproc-per-node 1`` -- RCCL
    initialisation, the barrier / max-reduce timing path and the hand-over collective all run (world size 1);
  * two host threads stepping through ONE plan concurrently (own streams, own workspaces), including the
    graph-replay path that mutates plan-owned state -- the contract stated in include/tcfd.h.
"""
import ctypes
import json
import os
import socket
import subprocess
import sys
import threading

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _torchrun(script_args, extra_env=None, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port())] + script_args
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_bench_under_torchrun_with_rccl():
    out = _torchrun(["bench.py", "--full", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-sfno", "--no-cpu-baseline",
                     "--no-probe", "--no-c4"], {"BENCH_FORCE_DIST": "1"})
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["value"] > 10 and out["scaling"] == "weak"
    assert out["roofline"]["bound"].startswith("hbm") and 0 < out["roofline"]["frac"] < 1
    assert out["roofline_worst"]["kernel"] in out["kernels"]
    assert out["launch"]["process_group"] is True and out["launch"]["rccl_world_size"] == 1
    assert out["strong_scaling"]["fields_per_gpu"] == [64] and out["strong_scaling"]["value"] > 10
    assert out["dram_bytes_per_step_est"] > 0 and out["dram_GBps_est"] < out["step_algo_GBps"]


def test_bench_strong_scaling_through_its_own_spawner():
    """`python bench.py --gpus 1 --scaling strong` with no launcher environment: the code path `--gpus 8` takes (the
    spawner only starts children for N > 1; N = 1 runs in place), headline = ONE batch cut across the ranks."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "bench.py", "--full", "--gpus", "1", "--scaling", "strong", "--steps", "3", "--warmup", "1",
                        "--no-sfno", "--no-cpu-baseline", "--no-probe", "--no-c4"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["scaling"] == "strong" and out["n_gpus"] == 1 and out["config"]["batch_total"] == 64 and out["value"] > 10
    assert out["strong_scaling"] is None and out["per_rank_steps_per_s"][0] == pytest.approx(out["value"], rel=1e-3)


def test_bench_c4_job_as_a_separate_process_tree():
    """What a multi-rank bench does with the C4 job: rank 0 starts it as its own set of ranks (`--c4-only` through the
    spawner) with a time limit and reads its JSON -- exercised here with one rank (BENCH_C4_SEPARATE=1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["BENCH_C4_SEPARATE"] = "1"
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--no-sfno", "--no-cpu-baseline",
                        "--no-probe", "--c4-samples", "8", "--batch", "4"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    c4 = json.loads(lines[0])["c4_ensemble"]
    assert "error" not in c4 and c4["finite"] is True and c4["seconds"] > 0
    # and a job that cannot finish in time is stopped, the bench line survives
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--no-sfno", "--no-cpu-baseline",
                        "--no-probe", "--c4-samples", "64", "--batch", "4", "--c4-timeout", "0.5"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][0])
    assert "did not finish" in out["c4_ensemble"]["error"] and out["value"] > 10


def test_bench_secondary_workloads_are_a_job_of_their_own():
    """The secondary workloads run as bench_secondary.py with a time limit after the headline; a few scalars reach the line (read
    the way the driver reads it: last brace-bearing line of stdout + stderr), the full record goes to the detail file; a job that
    cannot finish in time leaves the headline standing."""
    from test_bench_record import read_like_the_driver

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["BENCH_SECONDARY_ONLY"] = "notebook"
    cmd = [sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--regions", "3", "--no-cpu-baseline", "--no-probe",
           "--no-c4", "--batch", "8"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = read_like_the_driver(r.stdout.decode(), r.stderr.decode())
    assert out["value"] > 10 and len(out["timing"]["regions_ms_per_step"]) == 3 and 0 < out["roofline"]["frac"] < 1
    assert out["sfno_notebook_training"]["iterations_per_s"] > 10 and out["sfno_notebook_training"]["finite"] is True
    detail = json.load(open(os.path.join(ROOT, out["detail_file"])))
    assert detail["secondary"]["sfno_notebook_training"]["graph_replay"]["iterations_per_s"] > 10 and len(detail["regions"]) == 3
    r = subprocess.run(cmd + ["--secondary-timeout", "0.5"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = read_like_the_driver(r.stdout.decode(), r.stderr.decode())
    assert out["value"] > 10 and "did not finish" in out["secondary_error"]


def test_bench_c4_ensemble_line_small():
    """The C4 job line on one GPU with 16 samples: phases split out, dataset finite, hand-over through the pitched copies."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--no-sfno", "--no-cpu-baseline",
                        "--no-probe", "--c4-samples", "16", "--batch", "8"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][0])
    c4 = out["c4_ensemble"]
    assert "error" not in c4 and c4["finite"] is True and c4["seconds"] > 0
    assert c4["stepping_s"] > 0 and c4["handover_tail_s"] >= 0 and c4["dataset_GB"] == pytest.approx(16 * 10 * 4 * 256 * 256 * 4 / 1e9, rel=0.01)


def test_plain_bench_run_is_the_headline_and_its_outputs(tmp_path):
    """A run without --full: W + exactly K steps, the contract's keys, none of the --full measurements; --dump-outputs writes
    the last step's state and dw/dt in the run's precision, the same values run after run, a fixed sample of a large output."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}

    def run(*args):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1
        return json.loads(lines[0])

    outs = []
    for i in range(2):
        out = run("--steps", "4", "--warmup", "2", "--batch", "8", "--dump-outputs", str(tmp_path / f"d{i}"))
        assert out["steps"] == 4 and out["warmup"] == 2 and out["value"] > 10 and out["dtype"] == "f64" and out["full"] is False
        assert out["ms_per_step"] == pytest.approx(1e3 / out["value"], rel=1e-2) and out["higher_is_better"] is True
        assert out["metric"] and out["unit"].startswith("steps/s") and len(out["timing"]["regions_ms_per_step"]) == 1
        assert out["roofline"] is None and out["cpu_baseline"] is None
        for key in ("kernels", "strong_scaling", "strong_scaling_proxy", "hbm_probe", "c4_ensemble", "fused_steps_api",
                    "detail_file"):
            assert key not in out, key
        outs.append({name: np.load(tmp_path / f"d{i}" / f"{name}.npy") for name in ("w", "dwdt")})
    for name in ("w", "dwdt"):
        a, b = outs[0][name], outs[1][name]
        assert a.dtype == np.float64 and a.shape == (2 ** 20, 2) and np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b), name
    out = run("--steps", "2", "--warmup", "1", "--n", "64", "--batch", "4", "--dtype", "f32", "--dump-outputs", str(tmp_path / "s"))
    w = np.load(tmp_path / "s" / "w.npy")
    assert out["dtype"] == "f32" and w.dtype == np.float32 and w.shape == (4 * 64 * 33, 2)
    assert out["outputs"]["shapes"]["w"] == [4 * 64 * 33, 2]


def test_record_handover_page_locks_every_region_once():
    """the host result of an ensemble job is page-locked region by region (one region = the rows of one batch in
    one field) from a helper thread.  With page-aligned fields and regions that are whole pages every lock covers exactly its
    region: all regions are locked, no warning fires, no two locks share a page, and the records land bit for bit."""
    import mmap
    import warnings

    from torch_cfd_amd.distributed import RecordHandover, batch_layout

    dev = torch.device("cuda:0")
    fields, total, batch, n_rec, ns = ("a", "b"), 6, 2, 2, 32          # a region: 2 x 2 x 32 x 32 floats = 16 KB = 4 pages
    layout = batch_layout(total, 1, batch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ho = RecordHandover(fields, total, n_rec, (ns, ns), torch.float32, layout, dev)
        for f in fields:
            assert ho.host[f].data_ptr() % mmap.PAGESIZE == 0
        recs = {}
        for start, count in layout[0]:
            for rec in range(n_rec):
                recs[(start, rec)] = torch.randn(count, len(fields), ns, ns, device=dev)
                ho.push(start, rec, recs[(start, rec)])
        ho.start_allocation()
        ho._alloc_thread.join()
        assert ho._alloc_error is None and not ho._lock_warned
        region = batch * n_rec * ns * ns * 4
        assert len(ho._registered) == len(fields) * len(layout[0])
        assert sorted(ho._registered) == sorted(ho.host[f][s0:s0 + 1].data_ptr() for f in fields for s0, _ in layout[0])
        assert all((b - a) >= region for a, b in zip(sorted(ho._registered), sorted(ho._registered)[1:]))
        full = ho.finish()
    for (start, rec), t in recs.items():
        for i, f in enumerate(fields):
            assert torch.equal(full[f][start:start + t.shape[0], rec], t[:, i].cpu())


def test_config4_example_under_torchrun_with_rccl():
    out = _torchrun(["examples/c4_mcwilliams_ensemble.py", "--per-gpu", "8", "--warmup-steps", "5", "--steps", "55",
                     "--record-every", "55"])
    assert out["process_group"] is True and out["finite"] is True
    assert out["shapes"]["vorticity"] == [8, 1, 256, 256] and out["shapes"]["random_states"] == [8]


@pytest.mark.parametrize("n,steps", [(64, 6), (256, 2)])   # 64^2: graph replay of the interior steps (mutable plan state)
def test_two_threads_share_one_plan(n, steps):
    import torch_cfd_amd as tc
    from oracle import ns2d as O

    dev = torch.device("cuda:0")
    torch.set_default_dtype(torch.float64)
    L = 2 * torch.pi
    grid = tc.Grid(shape=(n, n), domain=((0, L), (0, L)))
    op = tc.NavierStokes2DSpectral(1e-3, grid, drag=0.1, forcing_fn=tc.KolmogorovForcing(grid=grid, scale=1.0, wave_number=4),
                                   solver=tc.RK4CrankNicolsonStepper()).to(dev)
    B = 3
    fields = [torch.stack([torch.fft.rfft2(O.mcwilliams_vorticity(n, L, 4, 10 * t + s, torch.float64)) for s in range(B)]).to(dev)
              for t in range(2)]
    plan = op._plan(fields[0])
    lib = tc._lib.load()
    beta, gdt, mu = tc.RK4CrankNicolsonStepper.stage_scalars(op.solver.params, 1e-3)
    serial = [op(f, 1e-3, steps=steps)[0].clone() for f in fields]
    torch.cuda.synchronize()
    nbytes = lib.tcfd_ns2d_workspace_bytes(plan.handle, B)
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream(device=dev)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty_like(fields[i])
            with torch.cuda.device(dev):
                for _ in range(20):
                    rc = lib.tcfd_ns2d_step(plan.handle, fields[i].data_ptr(), out.data_ptr(), None, B, len(beta),
                                            tc._lib.darray(beta), tc._lib.darray(gdt), tc._lib.darray(mu), steps,
                                            1 / (steps * 1e-3), ws.data_ptr(), ws.numel(), ctypes.c_void_p(stream.cuda_stream))
                    if rc != 0:
                        raise RuntimeError(lib.tcfd_last_error().decode())
                stream.synchronize()
            results[i] = out
        except Exception as e:  # surfaced in the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    for i in range(2):
        assert torch.equal(results[i], serial[i])


def _two_ranks(mode, out, timeout):
    """Two ranks of tests/two_rank_one_gpu_worker.py, both on cuda:0; returns [(returncode, output)] per rank."""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   GLOO_SOCKET_IFNAME="lo", HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "two_rank_one_gpu_worker.py"), mode, out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    res = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()              # exactly the child started above
            o, _ = p.communicate()
            o += "\n[timeout]"
        res.append((p.returncode, o))
    return res


def test_two_ranks_share_the_one_device(tmp_path):
    """the record hand-over with a REAL peer on a one-GPU box.  (a) RCCL with two ranks on one device:
    expected to be refused at communicator creation ("Duplicate GPU detected", librccl) -- the test records which of the
    two outcomes happened and fails only on a third (a hang, a wrong answer).  (b) the staged form that does run here: a
    gloo group, DEVICE tensors, a peer's records staged through page-locked memory -- side stream, events, the pitched
    copies into the (sample, record) slots of the page-locked result all execute on the GPU; the two-rank dataset must equal
    the one-process dataset bit for bit (batch elements are independent trajectories)."""
    res = _two_ranks("rccl", str(tmp_path / "unused.pt"), 180)
    text = "\n".join(o for _, o in res)
    if all(rc == 0 for rc, _ in res):
        assert text.count("RCCL_TWO_RANKS_ONE_DEVICE_OK") == 2
        rccl = "ran"
    else:
        assert "[timeout]" not in text, text[-2000:]
        assert "uplicate GPU" in text or "invalid usage" in text.lower() or "ncclInvalidUsage" in text, text[-2000:]
        rccl = "refused (duplicate GPU)"
    print("RCCL, two ranks on one device:", rccl)
    out = str(tmp_path / "two_rank.pt")
    res = _two_ranks("staged", out, 600)
    for rc, o in res:
        assert rc == 0 and "STAGED_OK" in o, o[-3000:]
    two = torch.load(out)
    from torch_cfd_amd.data_gen import generate_mcwilliams_dataset

    torch.set_default_dtype(torch.float64)
    try:
        one = generate_mcwilliams_dataset(64, 6, 2, 1e-3, 4, 12, 4, random_state=3, subsample=2, device="cuda:0")
    finally:
        torch.set_default_dtype(torch.float32)
    assert sorted(one) == sorted(two)
    for k in one:
        assert one[k].shape == two[k].shape and torch.equal(one[k], two[k]), k
