"""Engineered clouds for the voxel-grid kernels' shared helpers (cvo_voxel_table.hpp): clouds whose cells sit where the open-addressing table
and the lane runs are at their hardest, which random clouds reach by chance or never.

  home_slot   a numpy mirror of the device's hash in uint64 arithmetic: two multiply-xorshift rounds, then ((h >> 32) * slots) >> 32.  The
              keys come from voxel_reading.cells.  tests/test_gpu_table_cases.py holds the mirror to the device's own function.
  homed       distinct integer cells whose home slot in a table of `slots` slots is the wanted one, found by searching a cube of cells that
              grows as far as it must; one point per cell, at a fixed offset inside the cell.
  simulate    sequential insertion of a cloud's cells, in index order, into a table: where each point's probe starts, how far it walks and
              whether it steps from the last slot to slot 0.  The kernels insert in no fixed order, so the table a kernel builds may differ;
              the set of occupied slots does not (linear probing fills the same slots whatever the order), and neither do the properties
              the cases are built for.

Every position is (c + u) * VOXEL with VOXEL a power of two and u a multiple of 1 / 64 in (0, 1): exact in float32, and x / VOXEL floors to c.
A reduction's table has 2 n slots for a cloud of n points, a fusion's 2 x the group's points, a map's 2 x max_rows."""
import functools

import numpy as np

import voxel_reading as vr

VOXEL = 0.25
OFFSET = 0.375                                                           # of a cell's one point (a second point of the cell: SECOND)
SECOND = 0.625
SIZES = (1, 2, 3, 64, 257)                                               # 257: two blocks, five waves
U64 = np.uint64


def home_slot(key, slots):
    """the slot at which the table starts to look for `key` (int64 or uint64 array), in a table of `slots` slots"""
    assert 1 <= int(slots) < 2 ** 32
    h = np.ascontiguousarray(key).astype(U64)
    with np.errstate(over="ignore"):
        h = h ^ (h >> U64(33)); h = h * U64(0xff51afd7ed558ccd)
        h = h ^ (h >> U64(33)); h = h * U64(0xc4ceb9fe1a85ec53)
        h = h ^ (h >> U64(33))
        return (((h >> U64(32)) * U64(int(slots))) >> U64(32)).astype(np.int64)


def positions(cells, offset=OFFSET):
    """(n, 3) float32: a point at `offset` (one value, or one per point and axis) inside each integer cell"""
    c = np.asarray(cells, np.float64).reshape(-1, 3)
    x = ((c + offset) * VOXEL).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), (c + offset) * VOXEL)    # exact
    return np.ascontiguousarray(x)


def keys_of(xyz, voxel=VOXEL):
    """(valid, key) of positions with zero features, by voxel_reading.cells"""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok, _, key = vr.cells(vr.points8(x, np.zeros((x.shape[0], 5), np.float32)), voxel)
    return ok, key


@functools.lru_cache(maxsize=4)
def cube(radius):
    """(cells (m, 3) int64, keys (m,) int64) of every integer cell of [-radius, radius]^3, in a shuffled order that is the same every time"""
    a = np.arange(-radius, radius + 1, dtype=np.int64)
    c = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    c = c[np.random.default_rng(1000 + radius).permutation(c.shape[0])]
    ok, key = keys_of(positions(c))
    assert ok.all()
    return c, key


def homed(homes, slots, avoid=()):
    """one distinct integer cell per entry of `homes`, cell i with home slot homes[i] in a table of `slots` slots; none of them in `avoid`
    (cells as rows or tuples).  (len(homes), 3) int64"""
    homes = np.asarray(homes, np.int64).reshape(-1)
    assert ((0 <= homes) & (homes < slots)).all()
    taken = {tuple(int(v) for v in c) for c in np.asarray(avoid, np.int64).reshape(-1, 3)}
    want = {int(h): int((homes == h).sum()) for h in np.unique(homes)}
    radius = 24
    while True:
        cells, key = cube(radius)
        home = home_slot(key, slots)
        found = {}
        for h, k in want.items():
            cand = [c for c in cells[home == h][:k + len(taken)].tolist() if tuple(c) not in taken][:k]
            if len(cand) < k:
                break
            found[h] = cand
        else:
            break
        radius *= 2
        assert radius <= 192, (slots, want)
    at = {h: 0 for h in want}
    out = np.zeros((homes.shape[0], 3), np.int64)
    for i, h in enumerate(homes.tolist()):
        out[i] = found[h][at[h]]; at[h] += 1
    assert len({tuple(c) for c in out.tolist()}) == out.shape[0]
    return out


def features(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 255.0, (n, 5)).astype(np.float32)


def simulate(key, valid, slots):
    """sequential insertion in index order.  dict(slot (n,) the slot of each point's cell (-1: invalid), home (n,), distance (n,) slots walked
    from home, wraps (n,) steps from the last slot to slot 0, fresh (n,) bool: the point claimed the slot, table (slots,) key or -1)"""
    key = np.asarray(key, np.int64); n = key.shape[0]
    home = np.where(valid, home_slot(key, slots), -1)
    table = np.full(slots, -1, np.int64)
    slot = np.full(n, -1, np.int64); dist = np.zeros(n, np.int64); wraps = np.zeros(n, np.int64); fresh = np.zeros(n, bool)
    for i in range(n):
        if not valid[i]:
            continue
        s = int(home[i]); k = int(key[i])
        while table[s] != -1 and table[s] != k:
            if s + 1 == slots:
                s = 0; wraps[i] += 1
            else:
                s += 1
            dist[i] += 1
            assert dist[i] < slots
        fresh[i] = table[s] == -1
        table[s] = k; slot[i] = s
    return dict(slot=slot, home=home, distance=dist, wraps=wraps, fresh=fresh, table=table)


def chain_order(table, first):
    """the occupied slots of a table in probe order from slot `first`, until the first empty one"""
    out, s = [], int(first)
    while table[s] != -1 and len(out) < table.shape[0]:
        out.append(s); s = 0 if s + 1 == table.shape[0] else s + 1
    return out


# ---- the cases.  Each returns dict(xyz (n, 3), feat (n, 5), cells (n, 3) the intended integer cell of each point (where valid), homes (n,)
# the intended home slot at `slots`, slots, name)
def _case(name, cells, homes, slots, offset, seed):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    return dict(name=name, xyz=positions(cells, offset), feat=features(cells.shape[0], seed), cells=cells,
                homes=np.asarray(homes, np.int64).reshape(-1), slots=int(slots))


def last_slot(n, slots=None, avoid=()):
    """n distinct cells all homed at the table's last slot: every insert but one steps from the last slot to slot 0, and the chain is n long"""
    slots = 2 * n if slots is None else slots
    homes = np.full(n, slots - 1, np.int64)
    return _case(f"last_slot_{n}", homed(homes, slots, avoid), homes, slots, OFFSET, 100 + n)


def one_slot_twice(n, slots=None):
    """ceil(n / 2) distinct cells homed at one slot in the table's middle, then the first floor(n / 2) of them once more: each second occurrence
    finds its own key as deep in the chain as its first one went, and for n > 64 from another wave"""
    slots = 2 * n if slots is None else slots
    m = (n + 1) // 2
    cells = homed(np.full(m, slots // 2, np.int64), slots)
    cells = np.concatenate([cells, cells[:n - m]])
    offset = np.concatenate([np.full((m, 3), OFFSET), np.full((n - m, 3), SECOND)])
    return _case(f"one_slot_twice_{n}", cells, np.full(n, slots // 2, np.int64), slots, offset, 200 + n)


def staircase(n, slots=None):
    """n distinct cells with homes h, h, h + 1, h + 1, ...: clusters that merge as they grow.  The homes start ceil(n / 4) slots before the
    table's end, so homes and chain both go on across the wrap"""
    slots = 2 * n if slots is None else slots
    steps = (n + 1) // 2
    homes = (slots - (steps + 1) // 2 + np.arange(n) // 2) % slots
    return _case(f"staircase_{n}", homed(homes, slots), homes, slots, OFFSET, 300 + n)


# the `runs` case: (cell number or None for an invalid point, run length), wave by wave
RUNS_WAVES = [
    [(0, 1), (1, 2), (2, 3), (3, 5), (4, 8), (5, 13), (6, 31), (7, 1)],          # wave 0: runs of 1, 2, 3, 5, 8, 13, 31, then 1 to fill it
    [(8, 64)],                                                                    # wave 1: one run of exactly 64
    [(9, 63), (10, 1)],                                                           # wave 2: a run that ends at lane 62, a run of 1 at lane 63
    [(11, 64)],                                                                   # wave 3 and lane 0 of wave 4: a run of 65 across the wave edge
    [(11, 1), (12, 4), (13, 3), (12, 5),                                          # wave 4 (the second block): A B A
     (14, 3), (None, 1), (14, 3),                                                 #   an invalid point inside a run
     (15, 2), (None, 2), (16, 2),                                                 #   invalid points between runs
     (0, 3), (8, 2), (0, 1),                                                      #   cells of earlier waves come back, and A B A again
     (17, 1), (18, 1), (17, 1), (18, 1),                                          #   A B A B one lane each
     (19, 28)],                                                                   #   a run to the wave's end ...
    [(19, 2), (None, 1), (20, 3), (12, 1)],                                       # ... that goes on in the last, partial wave of 7
]


def runs():
    """a cloud whose cell sequence is prescribed lane by lane (RUNS_WAVES): independent of the hash.  The points of a run differ inside the cell."""
    ids = [c for wave in RUNS_WAVES for c, length in wave for _ in range(length)]
    n = len(ids)
    assert [sum(length for _, length in w) for w in RUNS_WAVES] == [64] * 5 + [7] and n == 327
    rng = np.random.default_rng(400)
    cell_of_id = np.array([[k - 10, 2 * k - 7, -k] for k in range(21)], np.int64)
    cells = np.array([cell_of_id[c] if c is not None else [0, 0, 0] for c in ids], np.int64)
    offset = rng.integers(1, 64, (n, 3)) / 64.0
    xyz = positions(cells, offset)
    xyz[[c is None for c in ids]] = np.nan
    return dict(name="runs", xyz=xyz, feat=features(n, 400), cells=cells, ids=ids, homes=None, slots=2 * n)


def lane_run_lengths(key, valid):
    """what lane_runs sees: per wave of 64 points, [(lane at which a run starts, its length, its key or None for invalid points)]"""
    k = np.where(valid, np.asarray(key, np.int64), -1)
    out = []
    for w in range(0, k.shape[0], 64):
        wave, runs_, start = k[w:w + 64], [], 0
        for lane in range(1, wave.shape[0] + 1):
            if lane == wave.shape[0] or wave[lane] != wave[lane - 1]:
                runs_.append((start, lane - start, None if wave[start] < 0 else int(wave[start]))); start = lane
        out.append(runs_)
    return out


@functools.lru_cache(maxsize=1)
def all_cases():
    """every engineered case: the three table cases at each of SIZES, and `runs`"""
    return tuple([make(n) for make in (last_slot, one_slot_twice, staircase) for n in SIZES] + [runs()])


def split(case, parts):
    """the case as min(parts, n) posed members, contiguous pieces one after the other: ([(xyz, feat)], [4 x 4 pose]).  Each member is given in a
    frame of its own, shifted by whole voxels (exact in float32), and its pose shifts it back: the moved points are the case's points"""
    n = case["xyz"].shape[0]
    members, poses = [], []
    for m, idx in enumerate(np.array_split(np.arange(n), min(parts, n))):
        t = np.array([2 * m, -3 * m, m], np.float32) * np.float32(VOXEL)
        P = np.eye(4, dtype=np.float32); P[:3, 3] = t
        members.append((np.ascontiguousarray(case["xyz"][idx] - t), np.ascontiguousarray(case["feat"][idx]))); poses.append(P)
    return members, poses
