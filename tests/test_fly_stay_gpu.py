"""Lean re-entry of the flying waves (mc_roles.hip.h, option "fly_stay"), with full waves on the GPU.

A flying wave of the 2D role kernels that comes back to the rings may refill and re-enter its crossing loop without a full
scheduling round ("fly_stay" = N: up to N - 1 times between two full rounds; 1: never, the former schedule).  Which wave
runs a packet, and when, must not matter: frozen launches of 20 000 packets -- every flying lane refilled many times,
every ring used -- at "fly_stay" 1, 2 and a large value, grid_blocks 1 and 2, on the 20 x 10 and 13 x 5 grids, with and
without a dark zone, plain and with the random walk, give what the single-role kernel ("schedule" = 1) gives in the same
process, by the criteria of tests/test_fly_visit_gpu.py: counters, n_sent and the SED's packet counts equal, the absorbed
energy within the tolerance of tests/test_gpu_parity.py.  Lean re-entries are built into the padded kernels, so every
launch asks for them ("cell_key" = 1: the small disks are optically thick and would get the plain kernels) and checks that
it got them (get_info "fly_stay").  The small disks track the Stokes vector and hand their last packets over; Pascucci's
thin disk runs the headline's instantiation, neither.  A kernel that hands its last packets over (option "tail") still
does so with lean re-entries on, and a live launch conserves its packets and gives the temperature of "fly_stay" = 1
within the seed-to-seed scatter of two "fly_stay" = 1 launches, measured here."""
import copy
import inspect

import numpy as np
import pytest

from mcfost_amd.host import model as M

pytestmark = pytest.mark.gpu

N = 20000
LARGE = 1 << 20


def _dark(m):
    d = copy.copy(m)
    dz = np.zeros(m.n_cells, np.uint8)
    dz.reshape(m.cfg.nz, m.cfg.n_rad)[0:2, 4:12] = 1   # (the densest midplane cells, as test_frozen_parity_dark_zone)
    d.l_dark_zone = dz
    return d


def _walk(m):
    w = copy.copy(m)
    M.init_mrw(w)
    return w


def _models():
    small, s13 = M.build_model(M.small()), M.build_model(M.small(n_rad=13, nz=5))
    return {"small2d": small, "small13x5": s13, "small2d_dark": _dark(small), "small13x5_dark": _dark(s13),
            "small2d_mrw": _walk(small), "small13x5_mrw": _walk(s13), "small2d_dark_mrw": _walk(_dark(small)),
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
@pytest.mark.parametrize("stay", [1, 2, LARGE])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_dark", "small13x5_dark", "small2d_mrw", "small13x5_mrw",
                                  "small2d_dark_mrw", "pascucci"])
def test_lean_reentry_equals_single_role_kernel(reference, name, stay, grid_blocks):
    from mcfost_amd.engine import Engine
    m, prior, b = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e.set_option("fly_stay", stay)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=grid_blocks)
    assert e.get_info("fly_stay") == stay   # (the launch's kernel is one that takes lean re-entries)
    e.close()
    print(name, stay, grid_blocks, a["counters"])
    assert a["counters"]["packets"] == N and a["counters"]["crossings"] > 5 * N
    if "dark" in name:
        assert a["counters"]["dark_mirrors"] > 0
    _same(a, b, m)


@pytest.mark.parametrize("name", ["small2d", "small2d_mrw"])
def test_hand_over_is_taken_with_lean_reentries(reference, name):
    """k_thermal_roles_tail with a small threshold: the flying waves must see the hand-over (abort_flag 2) from a lean
    re-entry, put nothing down twice and lose nothing -- the tail kernel finishes exactly the packets that are left."""
    from mcfost_amd.engine import Engine
    m, prior, b = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e.set_option("fly_stay", LARGE)
    e.set_option("tail", 40)
    e.set_option("tail_where", 1)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    assert e.get_info("tail_where") == 1   # (the launch had a tail kernel, on the device)
    assert e.get_info("fly_stay") == LARGE
    e.close()
    _same(a, b, m)


def test_live_mode_conserves_packets_and_keeps_the_temperature():
    """Live mode reads the in-flight temperature from the partial folds, whose cadence per visit is unchanged.  The same
    seed at "fly_stay" = 1 and at a large value sends the same packets on the same emissions until the estimates differ;
    the two temperatures must then be closer to each other than two "fly_stay" = 1 launches of different seeds are (the
    scatter is measured here, over the cells that absorbed energy in all launches, as the rms of the relative difference)."""
    from mcfost_amd.engine import Engine
    m = M.build_model(M.small())
    runs = {}
    for key, stay, seed in (("a", 1, 8), ("b", 1, 9), ("lean", LARGE, 8)):
        e = Engine(m, N)
        e.set_option("cell_key", 1)   # (this disk is optically thick: the padded kernels, which take lean re-entries, on request)
        e.set_option("fly_stay", stay)
        r = e.run_thermal(N, seed=seed, grid_blocks=2)
        assert e.get_info("fly_stay") == stay
        runs[key] = (r, e.temp_finale(r["E_abs"]))
        e.close()
        assert r["counters"]["packets"] == N and r["counters"]["escaped"] + r["counters"]["killed_star"] == N
    sel = (runs["a"][0]["E_abs"] > 0) & (runs["b"][0]["E_abs"] > 0) & (runs["lean"][0]["E_abs"] > 0)
    assert sel.sum() > m.n_cells // 2
    rms = lambda x, y: float(np.sqrt(np.mean((x[sel] / y[sel] - 1.0) ** 2)))
    scatter, diff = rms(runs["b"][1], runs["a"][1]), rms(runs["lean"][1], runs["a"][1])
    print("rms relative temperature difference: seed to seed %.3e, lean against full rounds %.3e" % (scatter, diff))
    assert diff <= scatter
