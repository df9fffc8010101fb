#!/usr/bin/env python3
"""Rate probe: milliseconds per step of the staged direct-P_l loop (the bench's step shape: Nl = 3, resum + AP, reduce_Plk) at a batch of 128
for loop FFTLog sizes NFFT = 256, 384 and 512 (NonLinear(NFFT=...)).  One engine per size, the same draws for all; prints one JSON line.

    python tools/nfft_rates.py [--steps 200] [--warmup 40] [--batch 128] [--nfft 256 384 512]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def rate(NFFT, B, steps, warmup):
    import bench
    from eftpipe_amd import synth
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.parambasis import bias_row
    from eftpipe_amd.tables import EngineConfig

    k = synth.survey_kgrid(bench.NK)
    cfg = EngineConfig(Nl=3, k=k, NFFT=NFFT, with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, bench.Z)),
                       H_AP=float(synth.hubble(synth.OM_AP, bench.Z)))
    eng = Engine(cfg, max_batch=B)
    eng.set_plk_direct(True)
    d = synth.draw_batch(B, z=bench.Z, seed=7)
    bias = np.stack([bias_row(float(f), list(bench.BS), None, bench.ES, kmA=0.7, krA=0.25, ndA=4.5e-5) for f in d["f"]])
    mask, shape = eng.full_mask(reduce=True), (B, 3, bench.NK)
    t = eng.tables
    sizes = {"coefficients": int(t["Gc"].shape[1]), "anti_diagonals": int(t["ad"].shape[1]), "ad_table_MB": t["ad"].nbytes / 2**20,
             "synthesis_rows": [int(t["syn_k"].shape[0]), int(t["lin_k"].shape[0])]}

    def loop(n):
        for _ in range(n):
            eng.step(mask, d["Pin"], d["f"], d["DA"], d["H"], bias=bias, back=3, shape=shape)
        eng.flush()
        eng.sync()

    loop(warmup)
    t0 = time.perf_counter()
    loop(steps)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    eng.close()
    return dict(NFFT=NFFT, ms_per_step=ms, evaluations_per_s=B / ms * 1e3, **sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--nfft", type=int, nargs="+", default=[256, 384, 512])
    a = ap.parse_args()
    rows = [rate(n, a.batch, a.steps, a.warmup) for n in a.nfft]
    base = rows[0]["ms_per_step"]
    for r in rows:
        r["relative_to_first"] = r["ms_per_step"] / base
    print(json.dumps({"batch": a.batch, "steps": a.steps, "rates": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
