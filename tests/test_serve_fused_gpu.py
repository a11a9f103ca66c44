"""The fused serving round of the padded 2D role kernels (mc_roles.hip.h, FUSED), with full waves on the GPU.

A serving lane of these kernels bins its exited packet directly behind the SRV pop, keeps the record and emits the next
packet into it in the same round; a packet that leaves the grid later in the round stays the lane's record, state
S_EXITED, and is binned at the top of the lane's next serving round.  Which round bins or emits a packet must not matter:
frozen launches of 20 000 packets with the padded kernels on request ("cell_key" = 1: the small disks are optically thick
and would get the plain kernels, which keep the former round), each checking that its kernel ran the fused round
(get_info "serve_fused"), give what the single-role kernel ("schedule" = 1) gives in the same process, by the criteria of
tests/test_fly_stay_gpu.py: counters, n_sent and the SED's packet counts equal, the absorbed energy within the tolerance of
tests/test_gpu_parity.py.  The small disks track the Stokes vector and hand their last packets over; Pascucci's thin disk
runs the headline's instantiation, neither.  Also: a launch so small that the servers fly their flights in place, a launch
with a hand-over threshold set (the hand-over meets exits that wait for their capteur), and a live launch, which conserves
its packets."""
import numpy as np
import pytest

from mcfost_amd.host import model as M
from test_fly_stay_gpu import LARGE, N, _dark, _same, _walk

pytestmark = pytest.mark.gpu


def _models():
    small, s13 = M.build_model(M.small()), M.build_model(M.small(n_rad=13, nz=5))
    return {"small2d": small, "small13x5": s13, "small2d_dark": _dark(small), "small13x5_dark": _dark(s13),
            "small2d_mrw": _walk(small), "small13x5_mrw": _walk(s13), "pascucci": M.build_model(M.pascucci())}


@pytest.fixture(scope="module")
def reference():
    """Per model: (model, prior, the single-role kernel's frozen launches of N and of 1500 packets) -- computed once, left
    unchanged."""
    from mcfost_amd.engine import Engine
    out = {}
    for name, m in _models().items():
        e = Engine(m, N)
        e.set_option("schedule", 1)
        prior = e.run_thermal(2000, seed=1)["E_abs"]
        out[name] = (m, prior, e.run_thermal(N, seed=41, frozen=True, E_prior=prior),
                     e.run_thermal(1500, seed=43, frozen=True, E_prior=prior))
        assert e.get_info("serve_fused") == 0   # (the single-role kernel has no serving round)
        e.close()
    return out


@pytest.mark.parametrize("grid_blocks", [1, 2])
@pytest.mark.parametrize("stay", [1, 16])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_dark", "small13x5_dark", "small2d_mrw", "small13x5_mrw",
                                  "pascucci"])
def test_fused_serving_round_equals_single_role_kernel(reference, name, stay, grid_blocks):
    from mcfost_amd.engine import Engine
    m, prior, b, _ = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e.set_option("fly_stay", stay)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=grid_blocks)
    assert e.get_info("serve_fused") == 1   # (the launch's kernel is one that runs the fused round)
    assert e.get_info("fly_stay") == stay
    e.close()
    print(name, stay, grid_blocks, a["counters"])
    assert a["counters"]["packets"] == N and a["counters"]["crossings"] > 5 * N
    if "dark" in name:
        assert a["counters"]["dark_mirrors"] > 0
    if "mrw" in name:
        assert a["counters"]["mrw_walks"] > 0
    _same(a, b, m)


@pytest.mark.parametrize("name", ["small2d", "small13x5", "pascucci"])
def test_servers_that_fly_in_place(reference, name):
    """1500 packets in one workgroup: fewer owned lanes than half a wave, so the serving waves pop the FLY ring and fly
    those flights in place -- the ones that leave the grid there are exits the lane holds until its next round."""
    from mcfost_amd.engine import Engine
    m, prior, _, b = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    a = e.run_thermal(1500, seed=43, frozen=True, E_prior=prior, grid_blocks=1)
    assert e.get_info("serve_fused") == 1
    e.close()
    assert a["counters"]["packets"] == 1500
    _same(a, b, m)


@pytest.mark.parametrize("tail", [40, 400])
@pytest.mark.parametrize("name", ["small2d", "small2d_mrw"])
def test_hand_over_meets_held_exits(reference, name, tail):
    """k_thermal_roles_tail with a threshold: the workgroups hand over what they hold, owned records in state S_EXITED among
    them, and the tail kernel bins those -- exactly the packets that are left, nothing twice."""
    from mcfost_amd.engine import Engine
    m, prior, b, _ = reference[name]
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    e.set_option("fly_stay", LARGE)
    e.set_option("tail", tail)
    e.set_option("tail_where", 1)
    a = e.run_thermal(N, seed=41, frozen=True, E_prior=prior, grid_blocks=2)
    assert e.get_info("tail_where") == 1   # (the launch had a tail kernel, on the device)
    assert e.get_info("serve_fused") == 1
    e.close()
    _same(a, b, m)


@pytest.mark.parametrize("name", ["small2d", "pascucci"])
def test_live_launch_conserves_its_packets(name):
    from mcfost_amd.engine import Engine
    m = M.build_model(getattr(M, "small" if name == "small2d" else name)())
    e = Engine(m, N)
    e.set_option("cell_key", 1)
    r = e.run_thermal(N, seed=8, grid_blocks=2)
    assert e.get_info("serve_fused") == 1
    e.close()
    c = r["counters"]
    assert c["packets"] == N and c["escaped"] + c["killed_star"] == N
    assert float(np.sum(r["n_sent"])) == N
