"""The SED commit pass with its deposits as 16-byte records in the binned log (option "xi_log" = 3; mc_xirec.hip.h,
k_mono_rec, k_fold_xirec) against the CPU oracle and against the atomics it replaces: the same packets, the same SED
bins, xI_scatt to the project's tolerance for default-real records (test_sed_mode_default_real_records: the terms are the
same default-real products, summed in another order).  Small tuning values ("xi_rec_buckets", "xi_rec_fold_kb",
"xi_rec_log_mb") reach the paths a full-size run takes -- several buckets, a bucket folded by several workgroups, several
launches, regions that overflow -- on grids of a few hundred cells."""
import copy

import numpy as np
import pytest

from mcfost_amd.host import model as M
from helpers import sed_model, xI_close

pytestmark = pytest.mark.gpu

INFO = ("xi_rec_records", "xi_rec_folded", "xi_rec_drained", "xi_rec_overflow_blocks", "xi_rec_chunks", "xi_rec_buckets",
        "xi_rec_split", "xi_rec_log_bytes", "xi_log_records", "xi_log_chunks")
SMALL = {"xi_rec_buckets": 6, "xi_rec_fold_kb": 8}   # 18 000 sub-bins in 5 buckets of 4096, each folded by >= 2 workgroups
N_CHUNKS = 16


def _dark_model():
    """test_tail_kernel_frozen_parity's disk with a dark zone (the 40 most opaque cells away from the inner edge), with the
    SED step's emission tables as helpers.sed_model makes them."""
    from oracle import Oracle
    m = M.build_model(M.small(RT_n_incl=3, lsepar_pola=False))
    dz = np.zeros(m.n_cells, np.uint8)
    kf = m.kappa_factor.copy()
    kf[::m.cfg.n_rad] = 0.0
    dz[np.argsort(kf)[-40:]] = 1
    m.l_dark_zone = dz
    orc = Oracle(m, 50000)
    T = orc.temp_finale(orc.run_thermal(50000, seed=3, n_threads=1)["E_abs"])
    M.repartition_energie(m, T)
    m.extra["Tdust"] = T
    return m


MODELS = {
    "incl3": lambda: sed_model(M.small(RT_n_incl=3, lsepar_pola=False), n_thermal=50000),
    "incl3_nocontrib": lambda: sed_model(M.small(RT_n_incl=3, lsepar_pola=False, lsepar_contrib=False), n_thermal=50000),
    "incl1": lambda: sed_model(M.small(RT_n_incl=1, lsepar_pola=False), n_thermal=50000),
    "3d": lambda: sed_model(M.small(n_rad=10, nz=5, n_az=6, l3D=True, RT_n_incl=2, lsepar_pola=False), n_thermal=50000),
    "dark": _dark_model,
    "incl4": lambda: sed_model(M.small(RT_n_incl=4, lsepar_pola=False), n_thermal=50000),
    "incl3_pola": lambda: sed_model(M.small(RT_n_incl=3), n_thermal=50000),
}
_models, _refs = {}, {}


def _model(name):
    if name not in _models:
        _models[name] = MODELS[name]()
    return _models[name]


def _ref(name, lam, n2):
    """the oracle's run of (model, wavelength, packets per stream): computed once, shared, never written to"""
    key = (name, lam, n2)
    if key not in _refs:
        from oracle import Oracle
        _refs[key] = Oracle(_model(name), 1e5).run_mono(lam, n2, seed=3, n_chunks=N_CHUNKS, n_threads=8)
    return _refs[key]


def _engine(m, precision=4):
    from mcfost_amd.engine import Engine
    e = Engine(m, 1e5)
    e.set_rt1()
    e.set_xI_precision(precision)
    return e


def _run(e, lam, n2, options, **kw):
    for name, value in options.items():
        e.set_option(name, value)
    a = e.run_mono(lam, n2, seed=3, n_chunks=N_CHUNKS, **kw)
    return a, {k: e.get_info(k) for k in INFO}


def _check(a, b, cfg, xI=True):
    assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == b["counters"]
    assert np.array_equal(a["sed"][4], b["sed"][4])
    if xI:
        xI_close(a["xI_scatt"], b["xI_scatt"], rtol=1e-4, n_midplane_cells=0 if cfg.l3D else cfg.n_rad, atol_rel=1e-5)


def _check_split_of_records(i):
    """every record went exactly one way: summed by a fold, left in the staging at the end of a launch, or in a block that
    found its part of the log full"""
    assert i["xi_rec_records"] > 0
    assert i["xi_rec_records"] == i["xi_rec_folded"] + i["xi_rec_drained"] + 64 * i["xi_rec_overflow_blocks"], i


@pytest.mark.parametrize("name,lam,n2", [("incl3", 5, 40), ("incl3", 20, 40), ("incl3_nocontrib", 5, 40), ("incl1", 5, 40),
                                         ("3d", 4, 700), ("dark", 5, 40)])
def test_parity_with_the_oracle(name, lam, n2):
    m, b = _model(name), _ref(name, lam, n2)
    e = _engine(m)
    a, i = _run(e, lam, n2, dict(SMALL, xi_log=3))
    _check(a, b, m.cfg)
    _check_split_of_records(i)
    assert i["xi_rec_chunks"] >= 1 and i["xi_log_chunks"] == 0 and 2 <= i["xi_rec_buckets"] <= 6
    assert i["xi_rec_folded"] > 0
    if not m.cfg.l3D:
        assert i["xi_rec_split"] >= 2
    # every crossing with a deposit is a record of either log.  The sorted log's count ("xi_log" = 2) is what its waves
    # RESERVED, in blocks of 2048 with the unused entries padded: it bounds the records from above and cannot equal them.
    a2, i2 = _run(e, lam, n2, dict(xi_log=2))
    _check(a2, b, m.cfg)
    assert i2["xi_rec_records"] == 0 and i2["xi_rec_log_bytes"] == 0
    assert i["xi_rec_records"] <= i2["xi_log_records"] and i2["xi_log_records"] % 2048 == 0
    assert 0.5 * b["counters"]["crossings"] < i["xi_rec_records"] <= b["counters"]["crossings"]
    e.close()


def test_both_origins_are_reached():
    """(between the two wavelengths of the first case stellar and thermal records both occur)"""
    x5, x20 = _ref("incl3", 5, 40)["xI_scatt"], _ref("incl3", 20, 40)["xI_scatt"]
    assert x5[:, :, 2].sum() > 0 and x20[:, :, 4].sum() > 0       # N_type_flux = 5: star at n_Stokes + 2, thermal at + 4 (1-based)
    e = _engine(_model("incl3"))
    a5, _ = _run(e, 5, 40, dict(SMALL, xi_log=3))
    a20, _ = _run(e, 20, 40, {})
    assert a5["xI_scatt"][:, :, 2].sum() > 0 and a20["xI_scatt"][:, :, 4].sum() > 0
    e.close()


def test_overflow_and_several_launches():
    """The smallest log the option takes (1 MiB = 65 536 records): the pass's first launch -- 16 384 packets -- overflows its
    regions many times over, the following launches are cut to what the log holds.  Same outputs, same tolerance."""
    name, lam, n2 = "incl3", 5, 700
    m, b = _model(name), _ref(name, lam, n2)
    c = b["counters"]
    log_records, first = 65536, 16384
    cpp = c["crossings"] / c["packets"]            # records per packet: between half of this (asserted below) and this
    assert first * 0.5 * cpp > 4 * log_records                                    # the first launch: >= 4 logs of records
    assert c["packets"] > first + 4 * max(256.0, 0.6 * log_records / (0.5 * cpp))   # ... and >= 4 launches' worth behind it
    e = _engine(m)
    a, i = _run(e, lam, n2, dict(SMALL, xi_log=3, xi_rec_log_mb=1))
    _check(a, b, m.cfg)
    _check_split_of_records(i)
    assert i["xi_rec_log_bytes"] == 1 << 20
    assert i["xi_rec_chunks"] >= 3 and i["xi_rec_overflow_blocks"] > 0 and i["xi_rec_folded"] > 0
    assert 0.5 * c["crossings"] < i["xi_rec_records"] <= c["crossings"]
    # the records are the packets' crossings: the same number whatever the log's size
    a2, i2 = _run(e, lam, n2, dict(xi_rec_log_mb=0))
    _check(a2, b, m.cfg)
    _check_split_of_records(i2)
    assert i2["xi_rec_records"] == i["xi_rec_records"] and i2["xi_rec_log_bytes"] > 1 << 20
    e.close()


def test_launch_geometry():
    """One wave per workgroup (a wave flushes every block itself), few workgroups, many: the default geometry's outputs."""
    name, lam, n2 = "incl3", 5, 40
    m, b = _model(name), _ref(name, lam, n2)
    e = _engine(m)
    ref, i0 = _run(e, lam, n2, dict(SMALL, xi_log=3))
    _check(ref, b, m.cfg)
    for gb, bt in ((1, 64), (5, 128), (40, 256)):
        r, i = _run(e, lam, n2, {}, grid_blocks=gb, block_threads=bt)
        _check(r, ref, m.cfg)
        _check(r, b, m.cfg)
        assert np.allclose(r["sed"], ref["sed"], rtol=1e-10, atol=1e-10)
        _check_split_of_records(i)
        assert i["xi_rec_records"] == i0["xi_rec_records"]
    e.close()


@pytest.mark.parametrize("name,precision", [("incl4", 4), ("incl3_pola", 4), ("incl3", 8)])
def test_where_the_path_does_not_apply(name, precision):
    """More than three values per deposit (four observers; Stokes tracking) or FP64 records: "xi_log" = 3 runs as 0 does.
    (The atomics' order is not fixed: the packets, the counters and the SED bins are equal, xI_scatt agrees to the sums'
    rounding.)"""
    m = _model(name)
    lam, n2 = 5, 40
    e = _engine(m, precision)
    r0, i0 = _run(e, lam, n2, dict(xi_log=0))
    r3, i3 = _run(e, lam, n2, dict(SMALL, xi_log=3))
    for i in (i0, i3):
        assert i["xi_rec_records"] == 0 and i["xi_rec_chunks"] == 0 and i["xi_rec_log_bytes"] == 0 and i["xi_log_chunks"] == 0
    _check(r3, r0, m.cfg, xI=False)
    assert np.array_equal(r3["n_sent"], r0["n_sent"])
    if precision == 8:
        assert np.allclose(r3["xI_scatt"], r0["xI_scatt"], rtol=1e-9, atol=1e-12 * np.abs(r0["xI_scatt"]).max())
    else:
        xI_close(r3["xI_scatt"], r0["xI_scatt"], rtol=1e-4, n_midplane_cells=m.cfg.n_rad, atol_rel=1e-5)
    e.close()


def test_the_other_values_after_three():
    """"xi_log" = 0, 1 and 2 on a context that ran with 3: the record log's buffers are freed and each value does what it
    did (three observers: 1 picks the atomics, 2 the sorted log)."""
    from mcfost_amd.engine import McgpuError
    name, lam, n2 = "incl3", 5, 40
    m, b = _model(name), _ref(name, lam, n2)
    e = _engine(m)
    a, i = _run(e, lam, n2, dict(SMALL, xi_log=3))
    assert i["xi_rec_records"] > 0 and i["xi_rec_log_bytes"] > 0
    for value, sorted_log in ((0, False), (1, False), (2, True)):
        e.set_option("xi_log", 3)
        _, i = _run(e, lam, n2, {})
        assert i["xi_rec_log_bytes"] > 0
        a, i = _run(e, lam, n2, dict(xi_log=value))
        _check(a, b, m.cfg)
        assert i["xi_rec_log_bytes"] == 0 and i["xi_rec_records"] == 0 and i["xi_rec_chunks"] == 0
        assert (i["xi_log_chunks"] > 0) == sorted_log
    with pytest.raises(McgpuError):
        e.set_option("xi_log", 4)
    e.close()


def test_pipeline_two_wavelengths():
    """temperature_and_sed with "xi_log" = 3 against 0 from the same temperature step: the same packets and SED bins, the
    ray-traced dust SED from the two xI_scatt within 1e-4 of its maximum per wavelength."""
    from mcfost_amd.host import pipeline as P

    class OneThermalStep(P.EngineBackend):   # (both runs start from the same absorbed energies)
        cache = None

        def run_thermal(self, n, seed):
            if OneThermalStep.cache is None:
                OneThermalStep.cache = self.e.run_thermal(n, seed=seed)
            return OneThermalStep.cache

    m = copy.copy(_model("incl3"))
    m.extra = dict(m.extra)      # (the pipeline leaves its E_disk there)
    lams = [5, 20]
    e = _engine(m)
    e.set_option("xi_log", 0)
    r0 = P.temperature_and_sed(OneThermalStep(e), m, 100000, 40, lambdas=lams, seed=11, n_chunks=N_CHUNKS)
    for name, value in dict(SMALL, xi_log=3).items():
        e.set_option(name, value)
    r3 = P.temperature_and_sed(OneThermalStep(e), m, 100000, 40, lambdas=lams, seed=11, n_chunks=N_CHUNKS)
    assert e.get_info("xi_rec_records") > 0
    assert np.array_equal(r3["Tdust"], r0["Tdust"])
    # (the packet counts are integers and equal; the other SED arrays are FP64 sums of the same terms whose order no
    # launch fixes: test_sed_mode_packet_cap_and_launch_geometry's tolerance for two launches of the same packets)
    assert np.array_equal(r3["sed_mc"][4], r0["sed_mc"][4]) and np.array_equal(r3["n_sent"], r0["n_sent"])
    assert np.allclose(r3["sed_mc"], r0["sed_mc"], rtol=1e-10, atol=1e-10)
    for lam in lams:
        s0, s3 = r0["sed_rt"][lam - 1], r3["sed_rt"][lam - 1]
        assert s0.max() > 0 and np.abs(s3 - s0).max() <= 1e-4 * s0.max()
    e.close()
