"""The padded crossing's bookkeeping (fly_geom_2d<WALL = true>, mc_roles.hip.h), with full waves on the GPU.

tests/test_fly_geom_exact.py walks ONE emulated lane, in plain C, through the crossings; the device's own instructions -- the
v_sad_u32 of the layer step, the 24-bit multiply-add of the row's address in LDS, the sign bit put into the wall's register
in place -- run only in the kernel.  Frozen launches with the role kernel and option "cell_key" = 1 (the padded key and the
wall records whatever the disk's optical depth) against option "schedule" = 1 (the single-role kernel: plain index, the
specification's crossing) in the same process, packet for packet: the integer counters, n_sent and the packet counts of the
SED are equal, the absorbed energy agrees within the tolerance tests/test_gpu_parity.py sets between the role kernel and the
oracle in frozen mode.  The shapes: the 20 x 10 and 13 x 5 grids with Stokes tracking, the 20 x 10 grid without it and with
the random walk, Pascucci's thin 100 x 70 disk with 2e5 packets (the headline's instantiation), each at grid_blocks 1 and 2;
a launch that hands its last packets over (k_thermal_roles_tail); a launch of so few packets that the serving waves own
fewer than 32 lanes and fly long flights in place; and a live launch, which conserves its packets."""
import copy

import numpy as np
import pytest

from mcfost_amd.host import model as M
from test_fly_pad_gpu import _same

pytestmark = pytest.mark.gpu

N = 20000
N_FEW = 1500
SEED = 47


def _models():
    small = M.build_model(M.small())
    walk = copy.copy(small)
    M.init_mrw(walk)
    return {"small2d": (small, N), "small13x5": (M.build_model(M.small(n_rad=13, nz=5)), N),
            "small2d_nopola": (M.build_model(M.small(lsepar_pola=False)), N), "small2d_mrw": (walk, N),
            "small2d_few": (small, N_FEW), "pascucci": (M.build_model(M.pascucci()), 200000)}


@pytest.fixture(scope="module")
def reference():
    """Per shape: (model, packets, prior, the single-role kernel's frozen launch) -- computed once, left unchanged."""
    from mcfost_amd.engine import Engine
    out = {}
    for name, (m, n) in _models().items():
        e = Engine(m, n)
        e.set_option("schedule", 1)
        prior = e.run_thermal(2000, seed=1)["E_abs"]
        out[name] = (m, n, prior, e.run_thermal(n, seed=SEED, frozen=True, E_prior=prior))
        e.close()
    return out


def _padded(m, n, prior, options=(), **kw):
    from mcfost_amd.engine import Engine
    e = Engine(m, n)
    e.set_option("cell_key", 1)
    for k, v in options:
        e.set_option(k, v)
    a = e.run_thermal(n, seed=SEED, frozen=True, E_prior=prior, **kw)
    info = {"tail_where": e.get_info("tail_where")}
    e.close()
    return a, info


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_nopola", "small2d_mrw", "pascucci"])
def test_padded_bookkeeping_equals_single_role_kernel(reference, name, grid_blocks):
    m, n, prior, b = reference[name]
    assert bool(m.cfg.lsepar_pola) == (name not in ("small2d_nopola", "pascucci"))
    a, _ = _padded(m, n, prior, grid_blocks=grid_blocks)
    assert a["counters"]["packets"] == n and a["counters"]["crossings"] > 5 * n
    _same(a, b, m)


def test_hand_over(reference):
    """k_thermal_roles_tail: the flights put down at the hand-over were crossed by the padded form, the tail kernel goes on
    from their records with the specification's."""
    m, n, prior, b = reference["small2d"]
    a, info = _padded(m, n, prior, options=(("tail", 40), ("tail_where", 1)), grid_blocks=2)
    assert info["tail_where"] == 1   # (the launch had a tail kernel, on the device)
    _same(a, b, m)


def test_servers_fly_in_place(reference):
    """So few packets that a serving wave owns fewer than 32 lanes: it takes long flights from the flying waves' ring and
    crosses them in place, between records that the flying waves load with their walls."""
    m, n, prior, b = reference["small2d_few"]
    a, _ = _padded(m, n, prior, grid_blocks=1)
    assert a["counters"]["packets"] == n and a["counters"]["crossings"] > 5 * n
    _same(a, b, m)


def test_live_mode_conserves_packets():
    from mcfost_amd.engine import Engine
    m = M.build_model(M.small())
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    r = e.run_thermal(N, seed=8, grid_blocks=2)
    e.close()
    c = r["counters"]
    assert c["packets"] == N and c["escaped"] + c["killed_star"] == N and c["crossings"] > 5 * N
    assert np.all(np.isfinite(r["E_abs"])) and r["E_abs"].sum() > 0
