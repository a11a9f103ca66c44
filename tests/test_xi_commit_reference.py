"""The int64 reference of tests/xi_commit_cases.py against the product's own specification of a deposit, without a GPU.

The wave functions of the SED commit pass cannot run in the one-lane emulation, but the value-by-value forms of
deposit_rt1_wave under MCGPU_LANE_EMULATION can: the FP64 records and the packed default-real layout (xI_f32), with one
dust class and with class tables.  They get the same integer records as the GPU test (tests/test_xi_commit_exact.py), one
emulated lane after the other, and the array must EQUAL the numpy reference -- for every observer count of the GPU test,
with and without Stokes tracking and contributions.  So the reference places every value where the product does, and a
mismatch on the GPU points at the staging."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import xi_commit_cases as K
from mcfost_amd.engine import xi32_layout

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mcfost_amd", "csrc")
COMBOS = [(nRT, pola, contrib) for nRT in K.NRT_ALL for pola in (False, True) for contrib in (False, True)]


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "emu", "emu_xi_commit.cpp")
    so = os.path.join(HERE, "emu", "libemu_xi_commit.so")
    deps = [src, os.path.join(HERE, "emu", "emu_kernel.cpp"), os.path.join(HERE, "emu", "emu_conv.h")] + \
           [os.path.join(CSRC, h) for h in ("mc_mono.hip.h", "mc_xi32.hip.h", "mc_xirec.hip.h", "mc_binned.hip.h", "mc_device.hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    l = C.CDLL(so)
    l.emu_xi_commit.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 11 + [C.c_void_p] * 3
    return l


def test_layouts_of_the_observer_counts():
    for nRT in K.NRT_ALL:
        assert xi32_layout(nRT, True, True)["split"] == K.SPLIT_POLA[nRT], nRT
        assert xi32_layout(nRT, False, True)["split"] == K.SPLIT_NOPOLA[nRT], nRT


@pytest.mark.parametrize("classes", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("nRT,pola,contrib", COMBOS)
def test_reference_equals_the_value_by_value_forms(lib, nRT, pola, contrib, f32, classes):
    rng = np.random.default_rng([21, nRT, pola, contrib, f32, classes])
    n_az = 3 if nRT % 2 else 1
    sch = K.random_schedule(rng, 128, n_az, R=6, star_by_wave=True)
    it, cw, sw, S = K.angles_of(rng, sch, nRT, 3 if f32 else 7)
    cls, vtab, p_lambda = None, None, 1
    if classes:
        mu = np.full((6, K.NANG + 1), 99.0, np.float32)          # (never read)
        vtab = K.mueller(rng, 3, 2)
        cls = rng.integers(0, 3, K.N_CELLS).astype(np.int32)
        p_lambda = 2
        vals = K.values_from_angles(sch, it, cw, sw, S, vtab, pola, cls, p_lambda)
    else:
        mu = K.mueller(rng)
        vals = K.values_from_angles(sch, it, cw, sw, S, mu, pola)
    x0 = K.start_array(rng, f32, nRT, pola, contrib, n_az)
    want = K.reference(sch, vals, x0, f32, nRT, pola, contrib)
    # the deposits, each with the results of the flight it belongs to
    on = sch.on
    where = sch.where[on].copy()
    where[:, 3] &= 1
    a = [np.ascontiguousarray(x) for x in (where, sch.l[on].astype(np.float64), sch.carried(it)[on], sch.carried(cw)[on],
                                            sch.carried(sw)[on], sch.carried(S)[on], mu)]
    got = x0.copy()
    p = lambda x: None if x is None else x.ctypes.data
    rc = lib.emu_xi_commit(len(where), *[p(x) for x in a], K.NANG, nRT, int(pola), int(contrib), int(f32), K.N_CELLS, K.N_THETA, n_az,
                           3 if classes else 0, 2, p_lambda, p(cls), p(vtab), p(got))
    assert rc == 0
    assert np.array_equal(got, want)
    ns = K.n_sub(n_az)
    pad = ~K.mapped_places(f32, nRT, pola, contrib)
    assert np.array_equal(got[ns:], x0[ns:]) and np.array_equal(got[..., pad], x0[..., pad]) and (got != x0).any()


def test_weights_and_angles_give_the_same_values():
    """paths 1 and 2 get the flight's weights, paths 0 and 3 the angles: with weights made from the angles both references
    add the same numbers"""
    rng = np.random.default_rng(22)
    sch = K.random_schedule(rng, 64, 1, R=5)
    it, cw, sw, S = K.angles_of(rng, sch, 4, 3)
    mu = K.mueller(rng)
    one = sch.l.copy()
    sch.l[:] = 1.0
    w = K.values_from_angles(sch, it, cw, sw, S, mu, True).astype(np.float32)     # (per item: already the carried flight's)
    sch.l[:] = one
    w_items = np.where(sch.fresh[..., None, None], w, np.float32(1e30))
    assert np.array_equal(K.values_from_weights(sch, w_items), K.values_from_angles(sch, it, cw, sw, S, mu, True))
