"""The flying waves' crossing with the leave test at the commit (fly_visit_step_2d<..., PAD, WALL, LATE>, fly_leave_2d and
fly_key, mc_roles.hip.h), with full waves on the GPU.

tests/test_fly_leave_exact.py walks ONE emulated lane, in plain C, through whole flights; the device's own instructions --
the 24-bit multiply-add of the cell's key, v_fract_f64, the conversion without a floor in front -- and the schedule around
them -- flights picked up from the FLY ring, after a hand-over, kept across visits, in cells that nobody has tested yet -- run
only in the kernel.  Frozen launches with the role kernel and option "cell_key" = 1 (the padded kernels whatever the disk's
optical depth) against option "schedule" = 1 (the single-role kernel: plain index, the specification's crossing) in the same
process, packet for packet, by the criteria of tests/test_fly_pad_gpu.py.  The shapes: the 20 x 10 and 13 x 5 grids with and
without Stokes tracking, the 20 x 10 grid with the random walk, Pascucci's thin 100 x 70 disk with 2e5 packets (the headline's
instantiation), a launch of so few packets (1500) that the serving waves fly long flights in place, and a launch that hands
its last packets over -- each at grid_blocks 1 and 2 and at "fly_stay" 1 (every visit behind a full scheduling round) and 16
(lean re-entries: flights stay across visits).  With the configurations' own stars (1 or 2 solar radii, an inner edge at
1 AU) no packet of these launches meets the star again (the CPU oracle counts none), so two more shapes exercise the
per-visit kill accounting, in the loop and at pick-up: the 20 x 10 and the 13 x 5 grid around a star of 60 solar radii, 1500
packets each, where the test asserts that the reference launch killed packets at the star.

Around that star the ROLE kernels -- padded and plain alike, with the library of the commit before the leave test moved as
with this one -- do not reproduce the single-role kernel's E_abs to the frozen tolerance: counters, n_sent and the SED counts
are equal, and ONE cell differs, by 1.6e-7 of its value in one set of launches and 2.7e-6 in another (1500 and 20000
packets; profiles/r06_fly_leave_ab.log has the figures).  Two things were told apart: with option "tail" = 0 a role launch is reproducible to every digit, padded and
plain agree with each other to 1e-13, and both differ from the single-role kernel in that one cell; with the automatic tail
the last packets are finished by the library's host threads, which packets those are depends on the schedule, and the
difference moves from launch to launch.  Its cause is not known and is owed a diagnosis of its own.  The star shapes
therefore run with "tail" = 0 and are held two ways: counters (killed_star among them), n_sent and the SED against the
single-role kernel exactly, as everywhere else; E_abs against the PLAIN role kernel of the same launch options (device code
of the parent commit) at the frozen tolerance, which is the comparison of what this form changes.  Their E_abs against the
single-role kernel is printed and NOT asserted: no bound is known for it -- a bound of 1e-6 taken from the first
measurements was exceeded by the next launch -- and none will be until the cause is found.  The hand-over also runs around
the large star (device tail kernel) and is held there on the counters, n_sent and the SED.  One live launch conserves its packets and kills some."""
import copy

import numpy as np
import pytest

from mcfost_amd.host import model as M
from test_fly_pad_gpu import _same

pytestmark = pytest.mark.gpu

N = 20000
N_FEW = 1500
SEED = 53
R_STAR = 60.0   # solar radii (0.28 AU)


def _models():
    small = M.build_model(M.small())
    walk = copy.copy(small)
    M.init_mrw(walk)
    return {"small2d": (small, N), "small13x5": (M.build_model(M.small(n_rad=13, nz=5)), N),
            "small2d_nopola": (M.build_model(M.small(lsepar_pola=False)), N),
            "small13x5_nopola": (M.build_model(M.small(n_rad=13, nz=5, lsepar_pola=False)), N),
            "small2d_mrw": (walk, N), "small2d_few": (small, N_FEW), "pascucci": (M.build_model(M.pascucci()), 200000),
            "small2d_star": (M.build_model(M.small(R_star=R_STAR)), N_FEW),
            "small13x5_star": (M.build_model(M.small(n_rad=13, nz=5, R_star=R_STAR)), N_FEW)}


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


def _same_but_E_abs(a, b, m):
    """_same on everything but E_abs: counters, n_sent, the SED."""
    _same(dict(a, E_abs=b["E_abs"]), b, m)


def _padded(m, n, prior, stay, options=(), cell_key=1, **kw):
    from mcfost_amd.engine import Engine
    e = Engine(m, n)
    e.set_option("cell_key", cell_key)
    e.set_option("fly_stay", stay)
    for k, v in options:
        e.set_option(k, v)
    a = e.run_thermal(n, seed=SEED, frozen=True, E_prior=prior, **kw)
    info = {"tail_where": e.get_info("tail_where")}
    e.close()
    return a, info


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("stay", [1, 16])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_nopola", "small13x5_nopola", "small2d_mrw", "small2d_few",
                                  "pascucci", "small2d_star", "small13x5_star"])
def test_leave_at_the_commit_equals_single_role_kernel(reference, name, stay, grid_blocks):
    m, n, prior, b = reference[name]
    assert bool(m.cfg.lsepar_pola) == ("nopola" not in name and "pascucci" not in name)
    # (both ways to leave, in the reference)
    assert (b["counters"]["killed_star"] > 0) == name.endswith("_star") and b["counters"]["escaped"] > 0
    star = name.endswith("_star")
    a, _ = _padded(m, n, prior, stay, options=(("tail", 0),) if star else (), grid_blocks=grid_blocks)
    print(name, stay, grid_blocks, a["counters"])
    assert a["counters"]["packets"] == n and a["counters"]["crossings"] > 5 * n
    if not star:
        _same(a, b, m)
        return
    _same_but_E_abs(a, b, m)
    plain, _ = _padded(m, n, prior, stay, options=(("tail", 0),), cell_key=2, grid_blocks=grid_blocks)
    _same(a, plain, m)
    worst = np.max(np.abs(a["E_abs"] - b["E_abs"]) / (1e-9 * np.abs(b["E_abs"]) + 1e-11 * b["E_abs"].max()))
    print("E_abs against the single-role kernel, in units of the frozen tolerance (not asserted): %.3g" % worst)


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("stay", [1, 16])
@pytest.mark.parametrize("name", ["small2d", "small2d_star"])
def test_hand_over(reference, name, stay, grid_blocks):
    """k_thermal_roles_tail: the flights put down at the hand-over go on in the tail kernel, with the specification's
    crossing, from cells the flying form committed -- tested there or not.  Around the large star the packets of the launch
    are killed at the star by whichever kernel holds them; that one is killed right after the hand-over is not observed."""
    m, n, prior, b = reference[name]
    assert (b["counters"]["killed_star"] > 0) == name.endswith("_star")
    a, info = _padded(m, n, prior, stay, options=(("tail", 40), ("tail_where", 1)), grid_blocks=grid_blocks)
    if grid_blocks == 2 and name == "small2d":   # (the shape at which tests/test_fly_geom_gpu.py establishes that the launch has a tail kernel)
        assert info["tail_where"] == 1
    if not name.endswith("_star"):
        _same(a, b, m)
        return
    _same_but_E_abs(a, b, m)


def test_live_mode_conserves_packets():
    from mcfost_amd.engine import Engine
    m = M.build_model(M.small(R_star=R_STAR))
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    r = e.run_thermal(N, seed=8, grid_blocks=2)
    e.close()
    c = r["counters"]
    assert c["packets"] == N and c["escaped"] + c["killed_star"] == N and c["crossings"] > 5 * N
    assert c["killed_star"] > 0
    assert np.all(np.isfinite(r["E_abs"])) and r["E_abs"].sum() > 0
