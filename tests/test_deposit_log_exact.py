"""The deposit logs' staging and folds on the GPU, compared bit for bit (mcgpu_probe_bin_stage, mcgpu_probe_xi_sort_fold).

The LDS protocol of mc_binned.hip.h (bin_deposit / bin_settle / bin_flush_block / bin_drain), k_fold_bins, k_fold_xirec,
the plans k_plan_uniform / k_plan_bins and the sorted log's k_xi_segfold run here on records the test chooses, by whole
workgroups: every lane of eight waves in one bucket, waves with one active lane, rounds with nobody, a starved log, a
launch that ends on a half-full half-buffer, a plan made from a launch unlike the next one, a sub-bin across three chunks.

Every input is a small integer, so every partial sum is an integer below 2^24 (default real) or 2^53 (double) -- each test
asserts that on its reference --, the sum is the same in any order and the device's result must EQUAL an int64 sum made
with numpy: a record that is lost, doubled, stale or misplaced cannot pass.  There is no tolerance in this file.  Values
beyond the record's nRT observers are 1e30 and must arrive nowhere; the arrays start from non-zero integers and carry
slack rows behind their logical length that must come back unchanged."""
import numpy as np
import pytest

from mcfost_amd.engine import xi32_layout, xi32_offset
from mcfost_amd.host import model as M

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF          # the key of "no record": the lane is inactive in that round
STAR = 0x80000000
N_OUT, SHIFT, N_BUCKETS = 18000, 12, 5     # 5 buckets of 4096 over 18 000 places: the last bucket is cut
SLACK = 7


@pytest.fixture(scope="module")
def eng():
    """one small engine: the probes use its context (device, stream) and none of its tables"""
    from mcfost_amd.engine import Engine
    e = Engine(M.build_model(M.small()), 1000)
    yield e
    e.close()


def records(rng, kind, keys, nRT=3):
    """integer values in [1, 8] for the records `keys` (NONE: no record); kind 1: a random origin in bit 31 of the key and
    1e30 in the values no observer has"""
    keys = np.asarray(keys, np.uint32).copy()
    n = keys.size
    if kind == 0:
        return keys, rng.integers(1, 9, n).astype(np.float64)
    vals = np.full((n, 3), 1e30, np.float32)
    vals[:, :nRT] = rng.integers(1, 9, (n, nRT))
    star = rng.random(n) < 0.4
    keys[(keys != NONE) & star] |= STAR
    return keys, vals


def start(rng, kind, n_alloc, nRT=3, contrib=True):
    if kind == 0:
        return rng.integers(1, 5, n_alloc).astype(np.float64)
    return rng.integers(1, 5, (n_alloc, xi32_layout(nRT, False, contrib)["binf"])).astype(np.float32)


def reference(kind, out0, keys, vals, n_out, nRT=3, contrib=True):
    """out0 + the records, in int64; kind 1: a record with its sub-bin beyond n_out is dropped"""
    acc = out0.astype(np.int64)
    on = keys != NONE
    if kind == 0:
        np.add.at(acc, keys[on].astype(np.int64), vals[on].astype(np.int64))
        assert np.abs(acc).max() < 2 ** 53
        return acc.astype(np.float64)
    sub = (keys & 0x7FFFFFFF).astype(np.int64)
    on &= sub < n_out
    star = (keys & STAR) != 0
    for q in range(nRT):
        # (no Stokes tracking: value q is observer q's flux, I or -- with contributions -- the packet's origin)
        o_star = xi32_offset(nRT, False, contrib, q, 2 if contrib else 0)
        o_thermal = xi32_offset(nRT, False, contrib, q, 4 if contrib else 0)
        o = np.where(star[on], o_star, o_thermal)
        np.add.at(acc, (sub[on], o), vals[on, q].astype(np.int64))
    assert np.abs(acc).max() < 2 ** 24
    return acc.astype(np.float32)


def pad_rounds(keys, T):
    keys = np.asarray(keys, np.uint32)
    return np.concatenate((keys, np.full((-keys.size) % T, NONE, np.uint32)))


def run(eng, rng, kind, keys, grid, threads, total_blocks, n_out=N_OUT, n_buckets=N_BUCKETS, shift=SHIFT, nRT=3, contrib=True,
        n_dropped_max=0, **kw):
    """stage + fold `keys` (whole rounds of grid * threads lanes) and check what every case owes"""
    keys, vals = records(rng, kind, keys, nRT)
    out0 = start(rng, kind, n_out + SLACK, nRT, contrib)
    res = eng.probe_bin_stage(kind, keys, vals, out0, grid, threads, n_buckets, shift, total_blocks, n_out, nRT=nRT,
                              contrib=contrib, **kw)
    want = reference(kind, out0, keys, vals, n_out, nRT, contrib)
    assert res["out"].dtype == want.dtype and res["out"].shape == want.shape
    assert np.array_equal(res["out"], want)
    assert np.array_equal(want[n_out:], out0[n_out:])                    # (the slack rows: untouched)
    made = int(np.count_nonzero(keys != NONE))
    assert res["made"] == made
    arrived = res["folded"] + res["drained"] + 64 * res["overflow"]
    assert made - n_dropped_max <= arrived <= made    # (n_dropped_max: records beyond n_out, which the fold drops uncounted)
    assert res["drained"] <= 63 * n_buckets * grid * kw.get("n_launches", 1)
    assert not res["counts_left"].any()
    for off, cap in zip(res["off"].astype(np.int64), res["cap"].astype(np.int64)):
        check_plan(off, cap, grid, total_blocks)
    res["made_by_test"] = made
    return res


def check_plan(off, cap, grid, total_blocks):
    end = off + cap * grid
    assert np.all(np.diff(off) >= 0) and np.all(end[:-1] <= off[1:]) and end[-1] <= total_blocks


KINDS = pytest.mark.parametrize("kind", [0, 1])


@KINDS
def test_uniform(eng, kind):
    """8 workgroups of 256 threads, 100 full rounds, keys uniform over the 18 000 places, a roomy log: nothing overflows,
    nearly everything is folded"""
    rng = np.random.default_rng(1)
    T = 8 * 256
    res = run(eng, rng, kind, rng.integers(0, N_OUT, 100 * T), 8, 256, 8000, split=8, slice_sub=1366)
    assert res["overflow"] == 0 and res["folded"] > 0.95 * res["made"]
    assert res["made"] == res["folded"] + res["drained"]


@pytest.mark.parametrize("kind,threads", [(0, 512), (0, 768), (1, 512)])
@pytest.mark.parametrize("one_place", [False, True])
def test_hot_bucket(eng, kind, threads, one_place):
    """Every record in bucket 2 (one_place: in one place of it): every bin_deposit of a workgroup reserves 8 or 12 blocks
    of a buffer of two, so most lanes wait for a half that is being flushed.  The log is roomy: exactness rests on the
    staging and the fold, not on the sink's atomics."""
    rng = np.random.default_rng(2)
    T = 4 * threads
    n = 100 * T
    keys = np.full(n, (2 << SHIFT) + 1234) if one_place else rng.integers(2 << SHIFT, 3 << SHIFT, n)
    res = run(eng, rng, kind, keys, 4, threads, 5 * 4 * 1300, split=8)
    assert res["overflow"] == 0 and res["made"] == n == res["folded"] + res["drained"]
    assert res["folded"] >= n - 63 * 4


@KINDS
@pytest.mark.parametrize("grid", [1, 3])
def test_one_wave_per_workgroup(eng, kind, grid):
    """64 threads per workgroup: a deposit that completes a block is flushed by the same wave at its next call"""
    rng = np.random.default_rng(3)
    T = 64 * grid
    res = run(eng, rng, kind, rng.integers(0, N_OUT, 300 * T), grid, 64, 5 * grid * 100, split=2)
    assert res["overflow"] == 0 and res["folded"] > 0


def ragged_masks(rng, T):
    """[rounds][T] who deposits: sparse, half, nobody, only lane 63 of every wave, everybody -- interleaved"""
    lane = np.arange(T) % 64
    kinds = [lambda: rng.random(T) < 1.0 / 64, lambda: rng.random(T) < 0.5, lambda: np.zeros(T, bool),
             lambda: lane == 63, lambda: np.ones(T, bool)]
    order = rng.permutation(np.repeat(np.arange(5), (60, 60, 10, 40, 10)))
    return np.array([kinds[k]() for k in order])


@KINDS
def test_ragged_waves(eng, kind):
    rng = np.random.default_rng(4)
    grid, threads = 4, 256
    T = grid * threads
    mask = ragged_masks(rng, T)
    keys = np.where(mask, rng.integers(0, N_OUT, mask.shape), NONE).ravel()
    res = run(eng, rng, kind, keys, grid, threads, 2000, split=3, slice_sub=4096)
    assert res["overflow"] == 0 and res["folded"] > 0


@KINDS
@pytest.mark.parametrize("tail", [1, 63])
def test_ragged_waves_end_on_a_part_filled_half(eng, kind, tail):
    """as above with every record in bucket 1, and a last round that leaves every workgroup `tail` records in a half:
    exactly those are drained"""
    rng = np.random.default_rng(5)
    grid, threads = 2, 128
    T = grid * threads
    mask = ragged_masks(rng, T)
    last = np.zeros(T, bool)
    for w in range(grid):
        have = int(np.count_nonzero(mask[:, w * threads:(w + 1) * threads]))
        last[w * threads + rng.permutation(threads)[:(tail - have) % 64]] = True
    mask = np.vstack((mask, last[None]))
    keys = np.where(mask, rng.integers(1 << SHIFT, 2 << SHIFT, mask.shape), NONE).ravel()
    res = run(eng, rng, kind, keys, grid, threads, 2000, split=1, slice_sub=1)
    assert res["overflow"] == 0 and res["drained"] == grid * tail
    assert res["folded"] == res["made"] - grid * tail


@KINDS
@pytest.mark.parametrize("blocks_per_part", [0, 1])
def test_starved_log(eng, kind, blocks_per_part):
    """A log smaller than one block per part (cap 0 everywhere: everything goes through overflow and drain), and one of
    exactly one block per part.  What the log held before (key 0x7FFFFFFF, values 1e30) is never read."""
    rng = np.random.default_rng(6)
    grid, threads = 3, 256
    T = grid * threads
    total = N_BUCKETS * grid - 1 if blocks_per_part == 0 else N_BUCKETS * grid
    res = run(eng, rng, kind, rng.integers(0, N_OUT, 40 * T), grid, threads, total, split=2)
    assert np.all(res["cap"] == blocks_per_part)
    assert res["overflow"] > 0 and res["made"] == res["folded"] + res["drained"] + 64 * res["overflow"]
    if blocks_per_part == 0:
        assert res["folded"] == 0
    else:
        # (bucket 4 is a tenth of the others: every part of the others fills its block)
        assert res["folded"] >= 64 * (N_BUCKETS - 1) * grid


def edge_keys(n_out):
    ks = [n_out - 1, 0]
    for b in range(1, N_BUCKETS):
        ks += [b << SHIFT, (b << SHIFT) - 1]
    return np.array(ks)


def test_key_edges_cells(eng):
    rng = np.random.default_rng(7)
    grid, threads = 2, 256
    keys = pad_rounds(rng.permutation(np.repeat(edge_keys(N_OUT), 700)), grid * threads)
    res = run(eng, rng, 0, keys, grid, threads, 1000, split=2)
    assert res["overflow"] == 0 and res["folded"] > 0


@pytest.mark.parametrize("nRT", [1, 2, 3])
@pytest.mark.parametrize("contrib", [False, True])
def test_key_edges_records(eng, nRT, contrib):
    """the buckets' first and last sub-bins and the array's last one, both origins, every layout the records serve --
    and sub-bins in the slack behind n_out, which the sink and the fold must both drop"""
    rng = np.random.default_rng(8)
    grid, threads = 2, 256
    beyond = np.arange(N_OUT, N_OUT + SLACK)
    keys = pad_rounds(rng.permutation(np.concatenate((np.repeat(edge_keys(N_OUT), 700), np.repeat(beyond, 150)))), grid * threads)
    n_beyond = beyond.size * 150
    res = run(eng, rng, 1, keys, grid, threads, 1000, nRT=nRT, contrib=contrib, slice_sub=1366, n_dropped_max=n_beyond)
    assert res["overflow"] == 0 and res["folded"] > 0
    # (with nothing overflowing, the records beyond n_out are dropped by the fold unless they were drained)
    assert res["made"] - res["folded"] - res["drained"] >= n_beyond - 63 * grid


@pytest.mark.parametrize("k,fold_threads,split", [(1, 256, 1), (4, 256, 1), (5, 256, 1), (8, 256, 1), (9, 256, 1),
                                                  (9, 256, 8), (9, 256, 4), (5, 256, 4), (9, 64, 1), (9, 1024, 1), (1, 1024, 8)])
def test_fold_geometry_cells(eng, k, fold_threads, split):
    """One workgroup of 64 threads deposits exactly 64 k records into bucket 3: k blocks in one part.  With four waves
    (fold_threads 256) k_fold_bins' second block in flight exists for k >= 5 and for every wave from k = 8 on; split 4 =
    grid_blocks + 3 and 8 leave workgroups without a part."""
    rng = np.random.default_rng(9)
    res = run(eng, rng, 0, rng.integers(3 << SHIFT, 4 << SHIFT, 64 * k), 1, 64, N_BUCKETS * 16, split=split, fold_threads=fold_threads)
    assert (res["folded"], res["drained"], res["overflow"]) == (64 * k, 0, 0)


@pytest.mark.parametrize("slice_sub,fold_threads", [(1366, 1024), (4096, 1024), (1, 128)])
def test_fold_geometry_records(eng, slice_sub, fold_threads):
    """slice_sub = ceil(4096 / 3): a bucket's last slice is short and the last bucket's slices are cut by n_out;
    4096: one workgroup per bucket; 1: a workgroup per sub-bin"""
    rng = np.random.default_rng(10)
    grid, threads = 4, 256
    res = run(eng, rng, 1, rng.integers(0, N_OUT, 20 * grid * threads), grid, threads, 2000, slice_sub=slice_sub,
              fold_threads=fold_threads)
    assert res["overflow"] == 0 and res["folded"] > 0


@KINDS
def test_several_launches(eng, kind):
    """Three launches on a small log.  Launch 1 never uses bucket 4; launch 2 puts 90 % of its records there, into the
    floor k_plan_bins leaves a bucket without counts (at most 8 blocks per workgroup), and overflows; launch 3 is uniform."""
    rng = np.random.default_rng(11)
    grid, threads, rounds = 4, 256, 60
    n = rounds * grid * threads
    first = rng.integers(0, 4 << SHIFT, n)
    second = np.where(rng.random(n) < 0.9, rng.integers(4 << SHIFT, N_OUT, n), rng.integers(0, 4 << SHIFT, n))
    third = rng.integers(0, N_OUT, n)
    res = run(eng, rng, kind, np.concatenate((first, second, third)), grid, threads, 1200, n_launches=3, split=8, slice_sub=2048)
    assert res["off"].shape == res["cap"].shape == (3, N_BUCKETS)
    assert 0 < res["cap"][1, 4] <= 8 and res["overflow"] > 0 and res["folded"] > 0
    assert res["made"] == 3 * n == res["folded"] + res["drained"] + 64 * res["overflow"]


def test_bad_arguments_launch_nothing(eng):
    from mcfost_amd.engine import McgpuError
    rng = np.random.default_rng(12)
    keys, vals = records(rng, 1, rng.integers(0, N_OUT, 256))
    out0 = start(rng, 1, N_OUT)
    with pytest.raises(McgpuError):     # 96 buckets of 16-byte records do not fit in LDS
        eng.probe_bin_stage(1, keys, vals, out0, 1, 256, 96, 8, 1000, N_OUT, nRT=3, contrib=True)
    with pytest.raises(McgpuError):     # not whole rounds
        eng.probe_bin_stage(1, keys[:200], vals[:200], out0, 1, 256, N_BUCKETS, SHIFT, 1000, N_OUT, nRT=3, contrib=True)
    keys[5] = N_OUT                      # a key beyond the allocation
    with pytest.raises(McgpuError):
        eng.probe_bin_stage(1, keys, vals, out0, 1, 256, N_BUCKETS, SHIFT, 1000, N_OUT, nRT=3, contrib=True)


# ---- the sorted log's fold --------------------------------------------------------------------------------------------------

def sorted_fold_case(eng, rng, n, n_bins, nRT, pola, contrib, run_lengths=(), pad_blocks=()):
    """n records (run_lengths: sub-bins that get exactly that many; the rest at random; pad_blocks: lengths of runs of
    unused entries, as a wave leaves behind what it reserved, put at random places of the unsorted log) -> the fold,
    against int64 sums placed by xi32_offset"""
    nv = 4 if pola else 1
    n_flights = 37
    sub = rng.integers(0, n_bins, n)
    at = 0
    for i, m in enumerate(run_lengths):
        sub[at:at + m] = (i * 7 + 3) % n_bins      # (distinct sub-bins while there are fewer runs than n_bins / 7)
        others = sub[at + m:]
        others[others == (i * 7 + 3) % n_bins] = (i * 7 + 4) % n_bins
        at += m
    sub = rng.permutation(sub)
    keys = sub.astype(np.uint32) | np.where(rng.random(n) < 0.4, STAR, 0).astype(np.uint32)
    flight = rng.integers(0, n_flights, n).astype(np.uint32)
    l = rng.integers(1, 9, n).astype(np.float32)
    rows = rng.integers(-4, 5, (n_flights, nv * nRT)).astype(np.float32)
    sentinel = eng.xi_log_sentinel(n_bins)
    assert sentinel >= n_bins and sentinel & (sentinel + 1) == 0
    for m in pad_blocks:        # (their flight is a valid one and their length 1e30: counted anywhere, they show)
        p = int(rng.integers(0, keys.size + 1))
        keys = np.concatenate((keys[:p], np.full(m, sentinel, np.uint32), keys[p:]))
        flight = np.concatenate((flight[:p], rng.integers(0, n_flights, m).astype(np.uint32), flight[p:]))
        l = np.concatenate((l[:p], np.full(m, 1e30, np.float32), l[p:]))
    binf = xi32_layout(nRT, pola, contrib)["binf"]
    x0 = rng.integers(1, 5, (n_bins, binf)).astype(np.float32)
    got = eng.probe_xi_sort_fold(keys, flight, l, rows, nRT, pola, contrib, n_bins, x0)
    on = keys != sentinel
    b, star = (keys[on] & 0x7FFFFFFF).astype(np.int64), (keys[on] & STAR) != 0
    li, w = l[on].astype(np.int64), rows[flight[on]].astype(np.int64)
    acc, mag = x0.astype(np.int64), x0.astype(np.int64)
    for q in range(nRT):
        for slot in range(nv):
            o = xi32_offset(nRT, pola, contrib, q, slot)
            if o >= 0:     # (-2: I is not stored where it is the sum of the two origins)
                np.add.at(acc, (b, o), li * w[:, q * nv + slot])
                np.add.at(mag, (b, o), li * np.abs(w[:, q * nv + slot]))
        if contrib:        # the copy of I at the packet's origin
            o = np.where(star, xi32_offset(nRT, pola, contrib, q, nv + 1), xi32_offset(nRT, pola, contrib, q, nv + 3))
            np.add.at(acc, (b, o), li * w[:, q * nv])
            np.add.at(mag, (b, o), li * np.abs(w[:, q * nv]))
    assert mag.max() < 2 ** 24          # every partial sum, in any order, is an integer a default real holds
    assert got.dtype == np.float32 and np.array_equal(got, acc.astype(np.float32))
    return acc


@pytest.mark.parametrize("n", [1, 7, 8, 9, 511, 512, 513, 200000])
def test_sorted_fold_sizes(eng, n):
    """the unroll (8) and the chunk (512) boundaries of k_xi_segfold in the record count"""
    sorted_fold_case(eng, np.random.default_rng(20 + n % 97), n, 1000, 3, False, True)


@pytest.mark.parametrize("n_bins", [1023, 1024, 1025])
@pytest.mark.parametrize("nRT,pola,contrib", [(3, False, True), (10, True, True), (10, True, False), (1, False, False), (13, True, True)])
def test_sorted_fold_runs_padding_layouts(eng, n_bins, nRT, pola, contrib):
    """Sub-bins with 7, 8, 9, 511, 512, 513 and 1500 records (the last one is flushed by three or four waves), blocks of
    unused entries through the unsorted log, the sentinel at both sides of a power of two, both origins mixed, every
    arrangement of the packed layout.  13 observers with Stokes tracking and contributions are 65 values per crossing: a
    second window of 64 lanes (blockIdx.y = 1), which the layout accepts."""
    rng = np.random.default_rng(30)
    sorted_fold_case(eng, rng, 30000, n_bins, nRT, pola, contrib, run_lengths=(7, 8, 9, 511, 512, 513, 1500, 1, 520),
                     pad_blocks=(1, 37, 64, 2048, 700, 5))


def test_sorted_fold_one_sub_bin(eng):
    """every record in one sub-bin of two: every wave of the fold flushes to the same place"""
    sorted_fold_case(eng, np.random.default_rng(40), 40000, 2, 3, False, True, run_lengths=(39990,))
