"""The wall records of the padded 2D role kernels (WallRec, mc_roles.hip.h), with full waves on the GPU.

tests/test_fly_wall_exact.py walks ONE emulated lane through the crossings; the table in HBM, the 16-byte gather of the
flying waves one crossing ahead of its use and the hand-over of flights between records and registers (flight_constants
loads the record of the cell a flight starts in) exist only in the kernel.  Frozen launches run with the role kernel and
option "cell_key" = 1 (the padded key, hence the wall records, whatever the disk's optical depth) against option
"schedule" = 1 (the single-role kernel: plain index, the wall formed at every crossing) in the same process, packet for
packet: the integer counters, n_sent and the packet counts of the SED are equal, the absorbed energy agrees within the
tolerance tests/test_gpu_parity.py sets between the role kernel and the oracle in frozen mode.  The grids: 20 x 10, 13 x 5,
one with a dark zone (those instantiations keep forming the wall in the loop, next to tables that now carry the records),
Pascucci's 100 x 70.

The two halves of a record have different sources -- the walls follow the grid, the factors the opacities -- so an engine
whose grid is set after its opacities and one whose opacities are replaced must each give what a fresh engine gives."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_fly_pad_gpu import _models, _same

pytestmark = pytest.mark.gpu

N = 20000
SEED = 43


@pytest.fixture(scope="module")
def reference():
    """Per model: (model, prior, the single-role kernel's frozen launch) -- computed once, left unchanged."""
    from mcfost_amd.engine import Engine
    out = {}
    for name, m in _models().items():
        e = Engine(m, N)
        e.set_option("schedule", 1)
        prior = e.run_thermal(2000, seed=1)["E_abs"]
        out[name] = (m, prior, e.run_thermal(N, seed=SEED, frozen=True, E_prior=prior))
        e.close()
    return out


def _padded(m, prior, **kw):
    from mcfost_amd.engine import Engine
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    a = e.run_thermal(N, seed=SEED, frozen=True, E_prior=prior, **kw)
    e.close()
    return a


@pytest.mark.parametrize("grid_blocks", [1, 3])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_dark", "pascucci"])
def test_wall_records_equal_single_role_kernel(reference, name, grid_blocks):
    m, prior, b = reference[name]
    a = _padded(m, prior, grid_blocks=grid_blocks)
    assert a["counters"]["packets"] == N and a["counters"]["crossings"] > 5 * N
    if name == "small2d_dark":
        assert a["counters"]["dark_mirrors"] > 0
    _same(a, b, m)


def test_grid_set_after_the_opacities(reference):
    """Setting the grid writes the walls anew; the factors must come back from the opacities the library was given."""
    from mcfost_amd.engine import Engine
    m, prior, _ = reference["small13x5"]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e._upload_grid_cyl(m)
    a = e.run_thermal(N, seed=SEED, frozen=True, E_prior=prior, grid_blocks=2)
    e.close()
    _same(a, _padded(m, prior, grid_blocks=2), m)


def test_opacities_replaced(reference):
    """New opacities write the factors anew, in both halves of every record; the walls stay."""
    from mcfost_amd.engine import Engine, _a, _p
    m, prior, _ = reference["small13x5"]
    m2 = copy.copy(m)
    m2.kappa_factor = np.asarray(m.kappa_factor, np.float64) * (0.5 + 0.25 * (np.arange(m.n_cells) % 3))
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    first = e.run_thermal(N, seed=SEED, frozen=True, E_prior=prior, grid_blocks=2)
    d = np.float64
    dark = None if m2.l_dark_zone is None else _p(_a(m2.l_dark_zone, np.uint8), C.c_ubyte)
    e._chk(e.lib.mcgpu_set_opacity(e.ctx, C.c_int(m2.n_lambda), _p(_a(m2.kappa, d), C.c_double),
                                   _p(_a(m2.kappa_abs_LTE, d), C.c_double), _p(_a(m2.albedo, np.float32), C.c_float),
                                   _p(_a(m2.kappa_factor, d), C.c_double), dark), "mcgpu_set_opacity")
    second = e.run_thermal(N, seed=SEED, frozen=True, E_prior=prior, grid_blocks=2)
    e.close()
    assert second["counters"] != first["counters"]   # (the changed opacity changes the walks)
    _same(second, _padded(m2, prior, grid_blocks=2), m2)
