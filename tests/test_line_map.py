"""Molecular line channel maps (emission_line_map, mol_transfer.f90:484-847; integ_ray_mol, optical_depth.f90:419-599) without
a GPU: the device's kernels (mcfost_amd/csrc/mc_line.hip.h) on one emulated lane (tests/emu/emu_line.cpp) against the
restatement over the oracle's operators (tests/line_walk.py), and known answers on both.

Tolerances: the project's for default-real results of ray walks -- rtol 2e-6 (column_cases.RTOL) and atol 1e-8 x the cube's
largest value (helpers.xI_close) -- with the same zero pattern, and n_capped == 0.  The condition on the inputs that makes
n_vpoints the same in every build of the arithmetic (dv / dv_line * 20 further than 1e-4 from a half-integer at every step)
is asserted here for every case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_cases as L
import line_walk as W
from mcfost_amd.engine import line_opts
from mcfost_amd.host import molecule as MOL
from oracle.binding import _a, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_line.cpp")
LIB = os.path.join(HERE, "emu", "libemu_line.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(os.path.dirname(HERE), "include", "mcgpu.h")] + \
       [os.path.join(HERE, "emu", f) for f in ("emu_kernel.cpp", "emu_conv.h", "cross_cell_literal.h")] + \
       [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def emu_line(lib, o, m, mol, method=2, npix=L.NPIX, ang_disque=0.0, **kw):
    """(spectrum, continu, n_capped, cap) of the emulated kernel, in the shapes of Engine.line_map."""
    vd = getattr(m, "variable_dust", None)
    npx = npy = npix if method == 2 else 1
    lo, keep = line_opts(mol, m.n_cells, int(vd["p_n_cells"]) if vd is not None else 1, float(m.cfg.distance), float(m.cfg.rin),
                         method, npx, npy, L.map_size(m), 1.0, **kw)
    nRT = m.rt["RT_n_incl"] * m.rt["RT_n_az"]
    spec = np.full((nRT, lo.nTrans, lo.n_speed, npy, npx), np.nan, np.float32)
    cont = np.full((nRT, lo.nTrans, npy, npx), np.nan, np.float32)
    capped, cap = C.c_ulonglong(99), C.c_int()
    az = _a(m.rt["tab_RT_az"], np.float32)
    rc = lib.emu_line_map(C.byref(o.cm), C.c_double(ang_disque), C.c_double(float(m.cfg.rout)), _p(az, C.c_float), C.byref(lo),
                          _p(spec, C.c_float), _p(cont, C.c_float), C.byref(capped), C.byref(cap))
    assert rc == 0
    del keep
    return spec, cont, capped.value, cap.value


@pytest.mark.parametrize("n_speed", L.N_SPEEDS)
@pytest.mark.parametrize("name", list(L.CASES))
def test_emulated_kernel_against_the_restatement(emu, name, n_speed):
    m, o, mol, want = L.case(name, n_speed)
    assert want["half_dist"] > 1e-4, want["half_dist"]              # the condition on the inputs
    spec, cont, capped, cap = emu_line(emu, o, m, mol)
    assert capped == 0 and want["longest"] < cap
    assert (want["spectrum"] > 0).sum() > 0.2 * want["spectrum"].size
    worst = max(L.compare(spec, want["spectrum"], (name, "spectrum")), L.compare(cont, want["continu"], (name, "continu")))
    h = want["hist"]
    print("%s n_speed %d: largest relative difference %.3g; longest walk %d crossings (cap %d); n_vpoints mean %.1f, 2: %d, 200: %d, "
          "between: %d; half-integer distance %.3g" % (name, n_speed, worst, want["longest"], cap,
                                                       (h * np.arange(h.size)).sum() / max(1, h.sum()), h[2], h[200], h[3:200].sum(),
                                                       want["half_dist"]))
    if name == "cyl2d_cold":
        assert h[2] > 0 and h[200] > 0 and h[3:200].sum() > 0
    if name == "voronoi":
        assert h[1] == h.sum()


def both(emu, name, mol, **kw):
    """The restatement's and the emulated kernel's (spectrum, continu) for changed tables: known answers are asked of both."""
    m, o, _, rays, paths = L.grid_case(L.CASES[name][0])
    want = W.cube_from_paths(m, mol, rays, paths, lonly_top=kw.get("lonly_top", False), lonly_bottom=kw.get("lonly_bottom", False))
    spec, cont, capped, _ = emu_line(emu, o, m, mol, **kw)
    assert capped == 0
    return [("restatement", want["spectrum"], want["continu"]), ("emulated kernel", spec, cont)]


@pytest.mark.parametrize("name", ["cyl2d", "voronoi"])
def test_far_wings_equal_the_continuum_bit_for_bit(emu, name):
    """Two extra channels so far out that sigma2_m1 v^2 > 1e4 in every cell: the profile is exactly 0 there."""
    ts = np.concatenate([[-4.0e7], MOL.tab_speed_rt(-L.VMAX, L.VMAX, 33), [4.0e7]])
    mol = L.tables(name, 35, tab_speed=ts)
    m = L.grid_case(L.CASES[name][0])[0]
    vmax = 2.0e5 + float(np.max(np.abs(L.kepler_speed(m))))
    assert np.all(np.asarray(mol["sigma2_phiProf_m1"]) * (4.0e7 - vmax) ** 2 > 1e4)
    for who, spec, cont in both(emu, name, mol):
        assert (cont > 0).sum() > 10, who
        for iv in (0, 34):
            assert np.array_equal(spec[:, :, iv].view(np.uint32), cont.view(np.uint32)), (who, iv)
        assert not np.array_equal(spec[:, :, 17], cont), who


def test_thick_isothermal_medium_without_dust(emu):
    """At the line centre of a thick, isothermal, dust-free medium at rest every pixel through it gives emissivite / kappa x
    the unit factor: to 1e-12 in double before the cast (the restatement's I0), to the comparison's tolerance after it."""
    name = "cyl2d"
    m, o, _, rays, paths = L.grid_case(name)
    mol = L.tables(name, 33)
    n = m.n_cells
    S = np.array([3.0e-15, 7.0e-15])
    mol["vfield"] = np.zeros(n, np.float32)
    mol["kappa_mol_o_freq"] = np.full((2, n), 1.0e-3)                 # x the profile's c / (sqrt(pi) dv) ~ 1e6: tau >> 1 per AU
    mol["emissivite_mol_o_freq"] = mol["kappa_mol_o_freq"] * S[:, None]
    mol["emissivite_dust"] = np.zeros((2, n))
    mol["kappa_abs_LTE"] = np.zeros((2, 1))
    prof = MOL.init_doppler_profiles(np.full(n, 30.0, np.float32), 28.0, 0.0)
    mol.update(prof)
    want = W.cube_from_paths(m, mol, rays, paths, raw=True)
    mid = 16
    assert np.asarray(mol["tab_speed"])[mid] == 0.0
    through = want["tau"][:, :, mid].min(axis=1) > 100.0               # (a ray that only clips the thin surface is not asked)
    assert through.sum() > 0.4 * through.size
    assert np.allclose(want["I0"][through][:, :, mid], S[None, :], rtol=1e-12, atol=0)
    sr = (rays["pixelsize"][0] / (float(m.cfg.distance) * W.PC_TO_AU)) ** 2
    spec, cont, capped, _ = emu_line(emu, o, m, mol)
    for who, sp in (("restatement", want["spectrum"]), ("emulated kernel", spec)):
        img = sp[:, :, mid].reshape(sp.shape[0], 2, -1)
        for q in range(sp.shape[0]):
            sel = through[rays["q"] == q]
            expect = (S * sr * np.asarray(mol["transfreq"]))[:, None] * np.ones(sel.sum())
            assert np.allclose(img[q][:, rays["ipix"][rays["q"] == q][sel]], expect, rtol=L.RTOL, atol=0), who
    assert not cont.any()


def test_optically_thin_channel_ratio(emu):
    """Optically thin, zero velocity, uniform temperature: the ratio of two channels of any pixel is
    exp(-(v_a^2 - v_b^2) sigma2_m1).  Tolerance: the restatement's own error on this ratio x 10."""
    name = "cyl2d"
    m, o, _, rays, paths = L.grid_case(name)
    mol = L.tables(name, 33)
    n = m.n_cells
    mol["vfield"] = np.zeros(n, np.float32)
    mol["emissivite_dust"] = np.zeros((2, n))
    mol["kappa_abs_LTE"] = np.zeros((2, 1))
    mol.update(MOL.init_doppler_profiles(np.full(n, 30.0, np.float32), 28.0, np.float32(200.0) ** 2))
    thick = W.cube_from_paths(m, mol, rays, paths, raw=True)["tau"].max()
    scale = 1.0e-5 / thick                                             # the thickest ray gets tau = 1e-5: thin, yet 1 - exp(-dtau) keeps digits
    mol["kappa_mol_o_freq"] = np.asarray(mol["kappa_mol_o_freq"]) * scale
    mol["emissivite_mol_o_freq"] = np.asarray(mol["emissivite_mol_o_freq"]) * scale
    ts = np.asarray(mol["tab_speed"])
    a, b = 16, 17
    ratio = float(np.exp(-(ts[a] ** 2 - ts[b] ** 2) * float(mol["sigma2_phiProf_m1"][0])))
    want = W.cube_from_paths(m, mol, rays, paths, raw=True)
    assert want["tau"].max() < 1e-4
    spec, _, _, _ = emu_line(emu, o, m, mol)
    # (the brighter pixels: in a faint one dtau of a cell is so small that 1 - exp(-dtau) has few digits left)
    lit = want["spectrum"][:, :, b] > 1e-3 * want["spectrum"][:, :, b].max()
    assert lit.sum() > 100
    own = np.max(np.abs(want["spectrum"][:, :, a][lit].astype(np.float64) / want["spectrum"][:, :, b][lit] / ratio - 1.0))
    tol = 10.0 * max(own, 2.0 ** -24)                                  # (no smaller than one rounding of a default real)
    for who, sp in (("restatement", want["spectrum"]), ("emulated kernel", spec)):
        r = sp[:, :, a][lit].astype(np.float64) / sp[:, :, b][lit]
        print(who, "largest error of the ratio", float(np.max(np.abs(r / ratio - 1.0))), "tolerance", tol)
        assert np.all(np.abs(r / ratio - 1.0) <= tol), who


@pytest.mark.parametrize("name", ["cyl2d", "cyl3d"])
def test_channel_subsets_give_the_same_bits(emu, name):
    """81 channels against a 17-channel sub-list: a channel's value does not depend on which others are asked for."""
    m, o, mol, want = L.case(name, 81)
    pick = np.array([0, 3, 7, 16, 17, 31, 40, 41, 50, 62, 63, 64, 65, 70, 77, 79, 80])
    sub = L.tables(name, 17, tab_speed=np.asarray(mol["tab_speed"])[pick])
    full = emu_line(emu, o, m, mol)[0]
    for who, spec, _ in both(emu, name, sub):
        ref = want["spectrum"] if who == "restatement" else full
        assert np.array_equal(spec.view(np.uint32), ref[:, :, pick].view(np.uint32)), who


def test_lonly_top_on_the_edge_on_view(emu):
    name = "cyl2d"
    mol = L.tables(name, 33)
    (_, ws, wc), (_, gs, gc) = both(emu, name, mol, lonly_top=True)
    L.compare(gs, ws, "lonly_top spectrum")
    L.compare(gc, wc, "lonly_top continu")
    m, o, mol0, full = L.case(name, 33)
    assert np.array_equal(wc, full["continu"])                        # the dust is not cut
    assert np.array_equal(gc, emu_line(emu, o, m, mol0)[1])
    assert (gs[1] < full["spectrum"][1]).sum() > 100                  # the near edge-on view loses its lower half's line


@pytest.mark.parametrize("l_sym_ima", [False, True])
def test_method1_against_the_fixed_order_sum(emu, l_sym_ima):
    name = "cyl2d"
    m, o, _, _, _ = L.grid_case(name)
    mol = L.tables(name, 33)
    rays = W.ray_starts(m, 1, l_sym_ima=l_sym_ima)
    paths = W.walk_paths(o, m, rays)
    assert paths["unfinished"] == 0
    want = W.cube_from_paths(m, mol, rays, paths)
    # (7200 rays: about 1e5 steps, so no choice of inputs keeps every step 1e-4 away from a half-integer as the cases of
    # line_cases.py do; the distance is printed.  A step's n_vpoints changes between two builds only where, besides, the
    # default real dv sits on a rounding boundary of the double it is cast from.)
    print("method 1: half-integer distance %.3g over %d steps" % (want["half_dist"], int(paths["n_steps"].sum())))
    spec, cont, capped, _ = emu_line(emu, o, m, mol, method=1, l_sym_ima=l_sym_ima)
    assert capped == 0 and spec.shape == (2, 2, 33, 1, 1)
    print("method 1: largest relative difference", max(L.compare(spec, want["spectrum"], "method 1 spectrum"),
                                                       L.compare(cont, want["continu"], "method 1 continu")))


def test_l_sym_ima_leaves_the_other_half_zero(emu):
    name = "cyl2d"
    m, o, mol, want = L.case(name, 33)
    spec, cont, _, _ = emu_line(emu, o, m, mol, l_sym_ima=True)
    half = L.NPIX // 2 + L.NPIX % 2
    L.compare(np.ascontiguousarray(spec[..., :half]), want["spectrum"][..., :half], "l_sym_ima spectrum")
    L.compare(np.ascontiguousarray(cont[..., :half]), want["continu"][..., :half], "l_sym_ima continu")
    assert not spec[..., half:].any() and not cont[..., half:].any()
