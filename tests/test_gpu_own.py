"""A refused eftb_create leaves nothing behind: the engine it had begun (streams and events, no memory yet) is destroyed on the failing exit
-- the one run of eftb_destroy on a half-built engine on real hardware -- and the process goes on as if the call had never been made."""
import numpy as np
import pytest

from eftpipe_amd import _lib as L
from eftpipe_amd import synth
from eftpipe_amd.engine import Engine
from eftpipe_amd.parambasis import bias_row
from eftpipe_amd.tables import EngineConfig

pytestmark = pytest.mark.gpu


def test_refused_create_leaves_the_process_as_it_was():
    z = 0.7
    cos = synth.cosmology(z=z, Om=0.3, h=0.68)
    cfg = EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, z)), H_AP=float(synth.hubble(synth.OM_AP, z)))
    Pin = np.stack([cos["Pin"], 1.1 * cos["Pin"]])
    bias = np.stack([bias_row(float(cos["f"]), [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], None, (0.26, 0.0, -0.93), kmA=0.7, krA=0.25, ndA=4.5e-5)] * 2)

    def plk():  # templates and P_l [2, 3, Nk] of an ordinary engine
        eng = Engine(cfg, max_batch=2)
        out = eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"], bias=bias)
        eng.close()
        return out

    before = plk()
    # the first buffer alone (P_lin, [max_batch][Nkin] doubles: 3.4 TB at Nkin = 200) cannot exist: the allocation is refused with an error
    # return, with the engine's streams and events already created
    with pytest.raises(L.EftbError, match=r"own_dev\(.*buf\[id\].*\) failed: .+ \(.*eftbird\.hip:\d+\)"):
        Engine(cfg, max_batch=2**31 - 1)
    after = plk()
    assert np.all(np.isfinite(before[1])) and np.any(before[1] != 0.0)
    assert np.array_equal(before[1], after[1])  # P_l
    assert np.array_equal(before[0], after[0])  # the templates
