"""Integer-valued deposits for the SED commit pass's deposit functions and their int64 reference, shared by
tests/test_xi_commit_exact.py (the wave functions on the GPU, mcgpu_probe_xi_commit) and tests/test_xi_commit_reference.py
(the value-by-value forms of deposit_rt1_wave in the one-lane emulation).

A SCHEDULE is what the lanes of a launch do: R rounds of T = grid x threads lanes; in round r lane g handles item r T + g.
Per item: whether the lane deposits (`on`) and into which sub-bin (icell, psup, phik), the path length l in [1, 7], whether
a new flight starts (`fresh`: the lane's per-lane results are rewritten first) and, per flight, its origin (`star`) and
its per-lane results.  Every lane starts a flight in round 0.  The per-lane results of an item that starts no flight are
filled with values that must never be read (99 / 1e30).

The reference carries every lane's flight forward through the rounds and adds, per deposit and observer, the same
expressions as deposit_rt1_wave (mc_mono.hip.h) in int64, placed with the Python mirrors xi32_offset / xi32_layout of the
packed layout (tests/test_xi32_layout.py pins them to the header) or into the 8-slot FP64 records."""
import numpy as np

from mcfost_amd.engine import xi32_layout, xi32_offset

N_CELLS, N_THETA, SLACK = 5, 2, 7
NANG = 6                     # scattering-angle bins 0..6
NRT_ALL = (1, 2, 3, 4, 5, 6, 8, 10, 11, 16)
N_ACT = (12, 13, 16, 17, 32, 33, 63, 64)      # both sides of every trip boundary of the staging loops (see the GPU test)

# Which arrangement xi32_layout yields with contributions (without: one part, I stored, nothing to arrange):
#   Stokes tracking:    split for nRT = 4, 8, 10, 11, 16 (4: 16 values fill the stellar line, the thermal origins take
#                       the next; 5 and 6: either arrangement is two lines per origin, so interleaved), interleaved (5
#                       values per observer, observers straddling lines from nRT = 4 values on) for 1, 2, 3, 5, 6
#   no Stokes tracking: split (nA = 0: [star x nRT | thermal x nRT from the next line]) for 10, 11, 16;
#                       interleaved (star, thermal per observer) for 1..8
# (test_layouts_of_the_observer_counts asserts both tables from xi32_layout)
SPLIT_POLA = {1: False, 2: False, 3: False, 4: True, 5: False, 6: False, 8: True, 10: True, 11: True, 16: True}
SPLIT_NOPOLA = {1: False, 2: False, 3: False, 4: False, 5: False, 6: False, 8: False, 10: True, 11: True, 16: True}


def n_sub(n_az):
    return N_CELLS * N_THETA * n_az


def lds_bytes(path, nRT, threads, pola, contrib):
    """the probe's LDS (mc_commit_probe.hip.h::xi_commit_probe_lds, mirrored to pick a workgroup size that fits)"""
    lay = xi32_layout(nRT, pola, contrib)
    rowf = 0
    if path == 2:
        rowf = (nRT * (4 if pola else 1) + 3) // 4 * 4 if lay["split"] else lay["binf"]
    b = threads * 64 + threads * 8
    if not rowf and pola:
        b += 2 * nRT * threads * 8
    b += 3 * nRT * 8
    b = (b + 15) // 16 * 16
    b += rowf * threads * 4 if rowf else nRT * threads * 4
    b += threads * 4 + 6 * (NANG + 1) * 4
    return (b + 15) // 16 * 16


def threads_that_fit(path, nRT, pola, contrib, want=512):
    t = want
    while lds_bytes(path, nRT, t, pola, contrib) > 160 * 1024:
        t //= 2
    assert t >= 64
    return t


class Schedule:
    def __init__(self, rng, on, fresh, n_az, star_by_wave=False, one_bin=None):
        """on, fresh: bool [R, T].  Sub-bins at random, or `one_bin` = (icell, psup, phik) for every deposit.
        star_by_wave: the flights of wave w are all stellar (w % 3 == 0), all thermal (1) or mixed (2)."""
        on, fresh = np.asarray(on, bool), np.asarray(fresh, bool).copy()
        fresh[0] = True
        R, T = on.shape
        self.R, self.T, self.n_az, self.on, self.fresh = R, T, n_az, on, fresh
        self.where = np.zeros((R, T, 4), np.int32)
        self.where[..., 0] = rng.integers(1, N_CELLS + 1, (R, T))
        self.where[..., 1] = rng.integers(1, N_THETA + 1, (R, T))
        self.where[..., 2] = rng.integers(1, n_az + 1, (R, T))
        if one_bin is not None:
            self.where[..., :3] = one_bin
        self.where[~on, :3] = 0
        star = rng.random((R, T)) < 0.5
        if star_by_wave:
            wave = (np.arange(T) // 64) % 3
            star[:, wave == 0] = True
            star[:, wave == 1] = False
        self.l = rng.integers(1, 8, (R, T)).astype(np.float32)
        # the flight every item belongs to: the round it started in
        self.flight = np.maximum.accumulate(np.where(fresh, np.arange(R)[:, None], -1), axis=0)
        self.star = np.take_along_axis(star, self.flight, axis=0)
        self.where[..., 3] = self.star.astype(np.int32) | (fresh.astype(np.int32) << 1)
        self.sub = ((self.where[..., 0] - 1) * N_THETA + (self.where[..., 1] - 1)) * n_az + (self.where[..., 2] - 1)

    def carried(self, x):
        """a per-item array -> per item, the values of the flight the item belongs to"""
        idx = self.flight.reshape(self.flight.shape + (1,) * (x.ndim - 2))
        return np.take_along_axis(x, np.broadcast_to(idx, x.shape), axis=0)


def weights_of(rng, sch, nRT, pola):
    """paths 1, 2: the flights' weights, integers in [-7, 7] with zeros; 1e30 where no flight starts"""
    nv = 4 if pola else 1
    w = rng.integers(-7, 8, (sch.R, sch.T, nRT, nv)).astype(np.float32)
    w[rng.random(w.shape) < 0.15] = 0.0
    w[~sch.fresh] = 1e30
    return w


def angles_of(rng, sch, nRT, smax):
    """paths 0, 3: itheta, cosw, sinw per (flight, observer) and the Stokes vector; garbage where no flight starts"""
    it = rng.integers(0, NANG + 1, (sch.R, sch.T, nRT)).astype(np.int32)
    cw = rng.integers(-1, 2, (sch.R, sch.T, nRT)).astype(np.float64)
    sw = rng.integers(-1, 2, (sch.R, sch.T, nRT)).astype(np.float64)
    S = rng.integers(-smax, smax + 1, (sch.R, sch.T, 4)).astype(np.float64)
    it[~sch.fresh] = NANG          # (an index must stay inside the tables even where it is never read)
    cw[~sch.fresh] = 99.0
    sw[~sch.fresh] = 99.0
    S[~sch.fresh] = 99.0
    return it, cw, sw, S


def mueller(rng, n_classes=0, n_lambda=2):
    """[6, NANG + 1] (or [6, n_classes, n_lambda, NANG + 1]): s11 in [1, 3], the five ratios in {-1, 0, 1}"""
    shape = (NANG + 1,) if not n_classes else (n_classes, n_lambda, NANG + 1)
    t = rng.integers(-1, 2, (6,) + shape).astype(np.float32)
    t[0] = rng.integers(1, 4, shape)
    return t


def values_from_angles(sch, it, cw, sw, S, mu, pola, cell_class=None, p_lambda=1):
    """int64 [R, T, nRT, nv]: deposit_rt1_wave's expressions for every item (those without a deposit are never placed)"""
    it, cw, sw, S = sch.carried(it).astype(np.int64), sch.carried(cw).astype(np.int64), sch.carried(sw).astype(np.int64), \
        sch.carried(S).astype(np.int64)
    l = sch.l.astype(np.int64)[..., None]
    mu = mu.astype(np.int64)
    if cell_class is None:
        col = [mu[t][it] for t in range(6)]
    else:
        cls = np.asarray(cell_class)[np.maximum(sch.where[..., 0], 1) - 1][..., None]
        col = [mu[t][cls, p_lambda - 1, it] for t in range(6)]
    s11 = col[0]
    S0, S1, S2, S3 = (S[..., k][..., None] for k in range(4))
    if not pola:
        return (l * S0 * s11)[..., None]
    s12, s22, s33, s34, s44 = -s11 * col[1], s11 * col[2], -s11 * col[3], -s11 * col[4], -s11 * col[5]
    C1, C4 = S0, S3
    C2 = cw * S1 + (-sw) * S2
    C3 = sw * S1 + cw * S2
    D1 = s11 * C1 + s12 * C2
    D2 = s12 * C1 + s22 * C2
    D3 = s33 * C3 + (-s34) * C4
    D4 = s34 * C3 + s44 * C4
    return np.stack((l * D1, l * ((-cw) * D2 + (-sw) * D3), l * ((-sw) * D2 + cw * D3), l * D4), axis=-1)


def values_from_weights(sch, w):
    return sch.carried(w).astype(np.int64) * sch.l.astype(np.int64)[..., None, None]


def start_array(rng, f32, nRT, pola, contrib, n_az):
    n = n_sub(n_az) + SLACK
    if f32:
        return rng.integers(1, 5, (n, xi32_layout(nRT, pola, contrib)["binf"])).astype(np.float32)
    return rng.integers(1, 5, (n, nRT, 8)).astype(np.float64)


def reference(sch, vals, x0, f32, nRT, pola, contrib):
    """x0 + every deposit, in int64; asserts the bound below which the device's sums are exact in any order"""
    acc = x0.astype(np.int64)
    nS = 4 if pola else 1
    on = sch.on
    sub, star = sch.sub[on], sch.star[on]
    v = vals[on]                       # [deposits, nRT, nv]
    for q in range(nRT):
        for t in range(nS):
            if f32:
                o = xi32_offset(nRT, pola, contrib, q, t)
                if o >= 0:             # (-2: I where it is the sum of the two origins, not stored)
                    np.add.at(acc, (sub, o), v[:, q, t])
            else:
                np.add.at(acc, (sub, q, t), v[:, q, t])
        if contrib:                    # the copy of I in the place of its origin: n_Stokes + 2 (star) / + 4 (thermal), 1-based
            if f32:
                o = np.where(star, xi32_offset(nRT, pola, contrib, q, nS + 1), xi32_offset(nRT, pola, contrib, q, nS + 3))
                np.add.at(acc, (sub, o), v[:, q, 0])
            else:
                np.add.at(acc, (sub, q, np.where(star, nS + 1, nS + 3)), v[:, q, 0])
    assert np.abs(acc).max() < (2 ** 24 if f32 else 2 ** 53)
    return acc.astype(x0.dtype)


def mapped_places(f32, nRT, pola, contrib):
    """bool mask over a sub-bin's default reals (or an FP64 record's 8 slots): the places some (observer, type) maps to"""
    nS = 4 if pola else 1
    types = list(range(nS)) + ([nS + 1, nS + 3] if contrib else [])
    if not f32:
        m = np.zeros(8, bool)
        m[types] = True
        return m
    m = np.zeros(xi32_layout(nRT, pola, contrib)["binf"], bool)
    for q in range(nRT):
        for t in types:
            o = xi32_offset(nRT, pola, contrib, q, t)
            if o >= 0:
                assert not m[o]
                m[o] = True
    return m


def fetched_reference(raw, nRT, pola, contrib, n_az):
    """what the fetch makes of the packed array: [N_CELLS, nRT, N_type_flux, N_THETA, n_az], I = star + thermal in int64"""
    nS = 4 if pola else 1
    ntf = nS + (4 if contrib else 0)
    r = raw[:n_sub(n_az)].astype(np.int64).reshape(N_CELLS, N_THETA, n_az, -1)
    out = np.zeros((N_CELLS, nRT, ntf, N_THETA, n_az), np.int64)
    for q in range(nRT):
        for t in range(ntf):
            o = xi32_offset(nRT, pola, contrib, q, t)
            if o >= 0:
                out[:, q, t] = r[..., o]
            elif o == -2:
                out[:, q, t] = r[..., xi32_offset(nRT, pola, contrib, q, nS + 1)] + r[..., xi32_offset(nRT, pola, contrib, q, nS + 3)]
    return out.astype(np.float64)


# ---- lane schedules ---------------------------------------------------------------------------------------------------
def lanes_mask(rng, T, count_of_wave):
    """bool [T]: in wave w, count_of_wave(w) lanes chosen at random"""
    m = np.zeros(T, bool)
    for w in range(T // 64):
        m[64 * w + rng.permutation(64)[:count_of_wave(w)]] = True
    return m


def edge_schedule(rng, T, n_az):
    """Round 0: every lane into ONE sub-bin.  Rounds 1-8: wave w deposits with N_ACT[(w + r) % 8] of its lanes, no new
    flights (every row survives the neighbours' deposits).  Rounds 9-16: per wave one of -- lane 0 alone, lane 37, lane 63,
    lanes 60-63 (which stage and, at K = 5, never serve), nobody (the early return, next to waves that deposit), everybody,
    nobody, lane 5 -- with new flights for a third of the lanes, depositing or not.  Rounds 17-24: 40 % of the lanes, new
    flights for 30 %.  Origins by wave: all stellar, all thermal, mixed."""
    R = 25
    on, fresh = np.zeros((R, T), bool), np.zeros((R, T), bool)
    on[0] = True
    for r in range(1, 9):
        on[r] = lanes_mask(rng, T, lambda w: N_ACT[(w + r) % 8])
    singles = ([0], [37], [63], [60, 61, 62, 63], [], list(range(64)), [], [5])
    for r in range(9, 17):
        for w in range(T // 64):
            on[r, 64 * w + np.array(singles[(w + r) % 8], int)] = True
        fresh[r] = rng.random(T) < 0.33
    on[17:] = rng.random((8, T)) < 0.4
    fresh[17:] = rng.random((8, T)) < 0.3
    sch = Schedule(rng, on, fresh, n_az, star_by_wave=True)
    sch.where[0, :, :3] = (3, 2, n_az)
    sch.sub[0] = ((3 - 1) * N_THETA + (2 - 1)) * n_az + (n_az - 1)
    return sch


def random_schedule(rng, T, n_az, R=32, p_on=0.4, p_fresh=0.3, star_by_wave=False):
    return Schedule(rng, rng.random((R, T)) < p_on, rng.random((R, T)) < p_fresh, n_az, star_by_wave=star_by_wave)
