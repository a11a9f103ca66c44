"""The padded cell key of the 2D role kernels (mc_roles.hip.h, PAD), with full waves on the GPU.

tests/test_fly_pad_exact.py walks ONE emulated lane through the crossings; the private grid in its padded layout -- the
zeroing, the deposits of 16 waves, the Temp_LTE reads, the rotating partial fold and the final fold -- and the padded
opacities in HBM exist only in the kernel.  Here frozen launches of 20 000 packets run with the default schedule (the role
kernel: padded key) at grid_blocks 1 and 2 against option "schedule" = 1 (the single-role kernel: plain index) in the same
process: the integer counters, n_sent and the packet counts of the SED are equal, the absorbed energy agrees within the
tolerance that tests/test_gpu_parity.py sets between the role kernel and the oracle in frozen mode.  The grids -- 20 x 10,
13 x 5 (a slot count that is no multiple of the waves of a workgroup), a dark zone, Pascucci's 100 x 70 -- send packets
through every halo: the hole, the layer above the disk, the outer edge, the midplane's mirror.

And the padded copy must follow the opacities: an engine whose kappa_factor is replaced gives what a fresh engine on the
changed model gives, and so does an engine whose grid is set again.  Option "cell_key" = 1 asks for the padded key on every model (by default a disk whose midplane is
optically thick keeps the plain kernels)."""
import copy
import ctypes as C
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
    return {"small2d": small, "small13x5": M.build_model(M.small(n_rad=13, nz=5)), "small2d_dark": dark,
            "pascucci": M.build_model(M.pascucci())}


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


def _same(a, b, m):
    """The criteria of tests/test_fly_visit_gpu.py between two frozen launches of the same packets."""
    from test_gpu_parity import _frozen_parity
    rtol = inspect.signature(_frozen_parity).parameters["rtol"].default   # (1e-9, with 1e-11 of the largest cell)
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    assert np.array_equal(a["n_sent"], b["n_sent"])
    assert np.array_equal(a["sed"][4], b["sed"][4])
    for t in (0, 5, 6, 7, 8):
        if m.cfg.lsepar_pola and m.cfg.aniso_method == 1:   # (update_Stokes renormalises I: 1 +- ulp per packet)
            assert np.allclose(a["sed"][t], b["sed"][t], rtol=1e-12, atol=1e-9), t
        else:
            assert np.array_equal(a["sed"][t], b["sed"][t]), t
    assert np.allclose(a["E_abs"], b["E_abs"], rtol=rtol, atol=1e-11 * b["E_abs"].max())


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_dark", "pascucci"])
def test_padded_role_kernel_equals_single_role_kernel(reference, name, grid_blocks):
    from mcfost_amd.engine import Engine
    m, prior, b = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)   # (padded whatever the disk's optical depth: these disks are thick, Pascucci's is not)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=grid_blocks)
    e.close()
    assert a["counters"]["packets"] == N and a["counters"]["crossings"] > 5 * N
    if name == "small2d_dark":
        assert a["counters"]["dark_mirrors"] > 0
    _same(a, b, m)


def test_padded_table_follows_the_opacities(reference):
    """A stale padded copy would leave the flights with the old kappa_factor while everything else reads the new one."""
    from mcfost_amd.engine import Engine, _a, _p
    m, prior, _ = reference["small2d"]
    m2 = copy.copy(m)
    m2.kappa_factor = np.asarray(m.kappa_factor, np.float64) * (0.5 + 0.25 * (np.arange(m.n_cells) % 3))
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    first = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    d = np.float64
    dark = None if m2.l_dark_zone is None else _p(_a(m2.l_dark_zone, np.uint8), C.c_ubyte)
    e._chk(e.lib.mcgpu_set_opacity(e.ctx, C.c_int(m2.n_lambda), _p(_a(m2.kappa, d), C.c_double),
                                   _p(_a(m2.kappa_abs_LTE, d), C.c_double), _p(_a(m2.albedo, np.float32), C.c_float),
                                   _p(_a(m2.kappa_factor, d), C.c_double), dark), "mcgpu_set_opacity")
    second = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    e.close()
    f = Engine(m2, N)
    f.set_option("cell_key", 1)
    fresh = f.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    f.close()
    assert second["counters"] != first["counters"]   # (the changed opacity changes the walks)
    _same(second, fresh, m2)


def test_padded_table_follows_the_grid(reference):
    """Setting the grid again discards the padded copies' layout; the library rebuilds them from the opacities it was given."""
    from mcfost_amd.engine import Engine
    m, prior, b = reference["small2d"]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e._upload_grid_cyl(m)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    e.close()
    _same(a, b, m)
