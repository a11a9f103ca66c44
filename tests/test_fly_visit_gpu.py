"""The flying loop's crossing under the flight predicate (fly_visit_step_2d), with full waves on the GPU.

tests/test_fly_visit_exact.py walks ONE emulated lane; a wrong exec mask -- a lane that commits what another lane's
branch computed, a lane that does not fly and loses a register -- shows only with 64 lanes whose flights end at
different iterations.  Here frozen launches of 20 000 packets run with the default schedule (the role kernel, whose
flying waves use the new crossing) at grid_blocks 1 and 2 -- full waves, every ring visited -- against option
"schedule" = 1 (the single-role kernel, which does not) in the same process: the integer counters, n_sent and the packet
counts of the SED are equal, the absorbed energy and the SED's fluxes agree within the tolerance that
tests/test_gpu_parity.py sets between the role kernel and the oracle in frozen mode (same packets, same random numbers,
another order of summation)."""
import copy
import inspect

import numpy as np
import pytest

from mcfost_amd.host import model as M

pytestmark = pytest.mark.gpu

N = 20000


def _models():
    small = M.build_model(M.small())
    dark = copy.copy(small)
    dz = np.zeros(small.n_cells, np.uint8)
    dz.reshape(small.cfg.nz, small.cfg.n_rad)[0:2, 4:12] = 1   # (the densest midplane cells, as test_frozen_parity_dark_zone)
    dark.l_dark_zone = dz
    return {"small2d": small, "pascucci": M.build_model(M.pascucci()), "small2d_dark": dark}


@pytest.fixture(scope="module")
def reference():
    """Per model: (model, prior, the single-role kernel's frozen launch) -- computed once, left unchanged."""
    from mcfost_amd.engine import Engine
    out = {}
    for name, m in _models().items():
        e = Engine(m, N)
        e.set_option("schedule", 1)
        prior = e.run_thermal(2000, seed=1)["E_abs"]
        out[name] = (m, prior, e.run_thermal(N, seed=41, frozen=True, E_prior=prior))
        e.close()
    return out


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("name", ["small2d", "pascucci", "small2d_dark"])
def test_role_kernel_equals_single_role_kernel(reference, name, grid_blocks):
    from mcfost_amd.engine import Engine
    from test_gpu_parity import _frozen_parity
    rtol = inspect.signature(_frozen_parity).parameters["rtol"].default   # (1e-9, with 1e-11 of the largest cell)
    m, prior, b = reference[name]
    e = Engine(m, N)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=grid_blocks)
    e.close()
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    assert a["counters"]["packets"] == N and a["counters"]["crossings"] > 5 * N
    if name == "small2d_dark":
        assert a["counters"]["dark_mirrors"] > 0
    assert np.array_equal(a["n_sent"], b["n_sent"])
    assert np.array_equal(a["sed"][4], b["sed"][4])
    for t in (0, 5, 6, 7, 8):
        if m.cfg.lsepar_pola and m.cfg.aniso_method == 1:   # (update_Stokes renormalises I: 1 +- ulp per packet)
            assert np.allclose(a["sed"][t], b["sed"][t], rtol=1e-12, atol=1e-9), t
        else:
            assert np.array_equal(a["sed"][t], b["sed"][t]), t
    assert np.allclose(a["sed"][1:4], b["sed"][1:4], rtol=1e-5, atol=1e-5 * max(1.0, np.abs(b["sed"][0]).max()))
    assert np.allclose(a["E_abs"], b["E_abs"], rtol=rtol, atol=1e-11 * b["E_abs"].max())
