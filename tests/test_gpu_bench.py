"""GPU: bench.py itself, as the driver launches it, in a FRESH child process (never a re-exec of this process, which has touched the GPU).

* the N > 1 loop of bench.py (RCCL gather -> gathered views -> drain -> slice checks) rehearsed on one GPU with EFTB_BENCH_FORCE_COMM=1:
  one rank exchanging with itself over RCCL.  Not a scaling measurement (DESIGN section 6 keeps saying "unmeasured").
* the N = 1 loop: every timed step bit-identical to the synchronous path, the dependent-sampler key present.
  Both read what only `--full` measures and checks.
* a plain run: the headline keys only, and --dump-outputs writes the P_l of the last timed step.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr

pytestmark = pytest.mark.gpu
FULL = ("--full", "--no-cpu-baseline", "--no-extras")


def _bench(extra_env, *flags):
    env = dict(os.environ, **extra_env)
    env.pop("EFTB_BENCH_DEPTH", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", *flags]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-1500:]
    return json.loads(lines[0])


def test_bench_multi_rank_loop_with_rccl_self_exchange():
    """bench.py's `exchange == "rccl"` loop: eftb_gather_plk every step, fetch_gathered(copy=False) views DEPTH steps back, the drain, and the
    asserts on the root's own slice of the gathered block (inside bench.py) -- all on one GPU."""
    j = _bench({"EFTB_BENCH_FORCE_COMM": "1"}, *FULL)
    assert j["valid"] is True and j["n_gpus"] == 1
    assert "rccl" in j["config"]["parallelism"]
    assert j["timed_steps_checked_against_sync_path"] == 4     # every timed step of the gathered loop == the synchronous path, bit for bit
    assert j["value"] > 0 and j["roofline"]["launches_timed"] >= 1


def test_bench_single_gpu_loop_checks_every_step():
    j = _bench({}, *FULL)
    assert j["valid"] is True and j["config"]["parallelism"] == "single GPU"
    assert j["timed_steps_checked_against_sync_path"] == 4
    assert j["sync_step_evaluations_per_s"] > 0 and j["sync_step_ms"] > 0
    assert 0.0 < j["roofline"]["frac"] < 1.0 and j["dtype"] == "f64"


def test_bench_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    """No --full: the result line carries the headline keys and nothing measured beside them, and --dump-outputs writes the P_l the timed loop
    delivered in its last step -- that of the draw set the arguments alone determine (step W + K - 1), as the synchronous path computes it."""
    import bench
    from eftpipe_amd import synth
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    j = _bench({}, "--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in j, key
    assert j["valid"] is True and j["steps"] == 4 and j["value"] > 0 and j["ms_per_step"] > 0
    assert not {"roofline", "cpu_baseline", "sync_step_ms", "templates_first_evaluations_per_s", "timed_steps_checked_against_sync_path"} & set(j)
    plk = np.load(tmp_path / "plk.npy")
    assert plk.dtype == np.float64 and plk.shape == (128, bench.NL, bench.NK) and np.all(np.isfinite(plk))
    cfg = EngineConfig(Nl=bench.NL, k=synth.survey_kgrid(bench.NK), with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, bench.Z)),
                       H_AP=float(synth.hubble(synth.OM_AP, bench.Z)))
    eng = Engine(cfg, max_batch=128, coalesce=bench.COALESCE)
    eng.set_latency_mode(False)
    eng.set_plk_direct(True)
    d = bench.draw_set(1 + 4 - 1, 128)
    want = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"], bias=d["bias"], templates=False)
    eng.close()
    assert relerr(plk, want) < 1e-12
