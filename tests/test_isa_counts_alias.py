"""Host: the entry of isa_counts.json that bench.py prices the direct resummation from describes the kernel that runs.

bench.py looks up "resum_plk_kernel<4,4>" and multiplies the hot loop's flops per wave and trip by 3 x 2 x 12 x 10 = 720 wave-trips per cosmology
(Nk = 512).  The kernel that runs is resum_plk_kernel<RSD_KPL, RSD_SH> with another geometry, so tools/isa_counts.py writes its counts under that
key rescaled; here the executed flops are recomputed from the real entry and the launch geometry of eftbird.hip and compared."""
import json
import os
import re
import sys

from conftest import ROOT

NK, NS = 512, 80
CSRC = os.path.join(ROOT, "eftpipe_amd", "csrc")


def test_bench_alias_prices_the_real_kernel():
    with open(os.path.join(CSRC, "isa_counts.json")) as fh:
        info = json.load(fh)
    with open(os.path.join(CSRC, "eftb_kernels.hpp")) as fh:
        kpl, sh = map(int, re.search(r"constexpr int RSD_KPL = (\d+), RSD_SH = (\d+);", fh.read()).groups())
    with open(os.path.join(CSRC, "eftbird.hip")) as fh:
        hip = fh.read()
    # the launch: one workgroup of 64 RSD_SH threads per (64 RSD_KPL k, cosmology)
    assert "resum_plk_kernel<RSD_KPL, RSD_SH>), dim3(nkd * B), dim3(64 * RSD_SH)" in hip and "nkd = (Nk + 64 * RSD_KPL - 1) / (64 * RSD_KPL)" in hip
    real = info[f"resum_plk_kernel<{kpl},{sh}>"]
    loop = max(real["loops"], key=lambda b: b["valu_f64"])
    waves = (NK + 64 * kpl - 1) // (64 * kpl) * sh       # per cosmology
    trips = NS // sh // 2                                # two s per trip of the loop
    executed = loop["flops_per_wave_trip"] * waves * trips
    # the source spells 118 FP64 vector instructions per (k, s): 37 for the basis, 9 x 8 for the dot products, 9 for H_v, all but 23 multiplies
    # FMAs.  The compiler may fuse or split a few, so this is a plausibility band (the Horner kernel issued 162): the check proper is the 1 % below
    assert 0.9 * 2 * kpl * 118 <= loop["valu_f64"] <= 1.1 * 2 * kpl * 118, loop["valu_f64"]
    assert 0.9 * NK * NS * (2 * 118 - 23) <= executed <= 1.1 * NK * NS * (2 * 118 - 23)
    alias = info["resum_plk_kernel<4,4>"]
    assert alias["alias_of"] == f"resum_plk_kernel<{kpl},{sh}>" and "note" in alias
    assert alias["unscaled"]["valu_f64"] == loop["valu_f64"] and alias["unscaled"]["wave_trips_per_cosmology"] == waves * trips
    aloop = max(alias["loops"], key=lambda b: b["valu_f64"])
    priced = aloop["flops_per_wave_trip"] * 3 * ((NK + 255) // 256) * 12 * (NS // 8)   # bench.py direct_step_flops, per cosmology
    print(f"executed {executed} flops per cosmology, priced by bench.py {priced:.1f}")
    assert abs(priced - executed) <= 0.01 * executed
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts

    assert isa_counts.resum_plk_shape() == (kpl, sh) and isa_counts.resum_plk_wave_trips(kpl, sh) == waves * trips
