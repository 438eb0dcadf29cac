"""The integer plan of a train step, as pinsage_engine_frontier leaves it in a
workspace, against int64 numpy (parity_util.frontier_plan_reference): the node
sets S_l / N_l of every layer (device counts, sorted members, read_counts), the
index tables loc / wloc / self_src / q_src, pos_rank and the position CSR
(rank_off, pos_sorted).  Everything is an integer or a bit copy: every
comparison is exact, wloc bit for bit.

The tests drive the real pinsage_engine_frontier / _forward_inference /
_read_counts on a real workspace of pinsage_model._Engine(n, 4, 4, 4, L, T,
max_pos) (the frontier reads neither features nor parameters; a dummy feature
tensor and zeroed parameters satisfy the pointer check) and read the plan
through pinsage_engine_offsets and pinsage_engine_plan_offsets.

Which kernels run is decided by the universe n (words = ceil(n / 64)), not by
the frontier's size; constants read off frontier.hip / conv.hip:

  words <= 8192 (n <= 524 288)        marking in a whole-bitmap LDS copy
  words <= 16384 (n <= 1 048 576)     sets finalised inside the marking launch
                                      (last workgroup by ticket, per = ceil(words
                                      / 1024) words per thread, 1 .. 16), top set
                                      in one block; above: multi-block scan and a
                                      multi-kernel top set
  20448-word LDS windows              1 window up to n = 1 308 672, 64 windows up
                                      to n = 83 755 008, global atomics beyond
  65536 ids per scan block            more than 256 blocks (n > 16 777 216): the
                                      strided block-offset loop runs
  n_pos <= 16384                      one-block radix sort of the positions;
                                      above: rank_off[0] = -1

Tables are built on the device: small universes a random permutation table,
large ones nb[i][t] = (i * a + off[t]) % n with distinct off[t] (every row's
first T entries distinct, all in [0, n): the engine's preconditions); wn holds
hashed bit patterns so a copy from the wrong slot shows.  Part of the cases use
a row stride ld > T.
"""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import POS_CSR_MAX, check_frontier_plan, frontier_plan_reference, perm_table

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
WIN_IDS = 20448 * 64      # ids per LDS marking window (kWinWords)
BLOCK_IDS = 65536         # ids per scan block (kWordsPerBlock words)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()  # (the large universes' tables are 0.67 GB each)


# ----------------------------------------------------------------------------- tables
def _hash_bits(i, t, seed):
    """int32 tensor of hashed 32-bit patterns (the float32 view is arbitrary)"""
    h = (i * 2654435761 + (t + 1) * 0x9E3779B1 + seed) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    return ((h ^ 0x80000000) - 0x80000000).to(torch.int32)


def arith_table(n, T, ld, a, seed):
    """nb[i][t] = (i * a + off[t]) % n, off[t] distinct and < n; wn: hashed bits"""
    assert n > 64 * ld
    offs = [(7 + 13 * seed + 53 * t * t + 11 * t) % n for t in range(ld)]
    assert len(set(offs)) == ld
    i = torch.arange(n, dtype=torch.int64, device=DEVICE)
    nb = torch.empty((n, ld), dtype=torch.int32, device=DEVICE)
    wb = torch.empty((n, ld), dtype=torch.int32, device=DEVICE)
    for t in range(ld):
        nb[:, t] = ((i * a + offs[t]) % n).to(torch.int32)
        wb[:, t] = _hash_bits(i, t, seed)
    return nb, wb


def plant_rows(nb, members, T):
    """rows of `members` point at each other, every member named by some row:
    nb[m[j]][t] = m[(j T + t + 1) % len(m)] (distinct within a row)"""
    m = np.asarray(members, np.int64)
    assert len(np.unique(m)) == len(m) >= T
    j = np.arange(len(m))[:, None] * T + np.arange(T)[None, :] + 1
    vals = torch.from_numpy(m[j % len(m)].astype(np.int32)).to(nb.device)
    nb[torch.from_numpy(m).to(nb.device), :T] = vals


def rows_of(tables, T):
    """rows(l, S) for the reference: the rows of S only, gathered on the device"""
    def rows(l, S):
        nb, wb = tables[l] if isinstance(tables, list) else tables
        s = torch.from_numpy(np.asarray(S, np.int64)).to(nb.device)
        return (nb[s, :T].cpu().numpy().astype(np.int64), wb[s, :T].cpu().numpy().view(np.uint32))
    return rows


def planted_ids(n):
    """ids on the edges the kernels cut the universe at (those below n)"""
    p = [0, n - 1, n - 2, 63, 64, BLOCK_IDS - 1, BLOCK_IDS, WIN_IDS - 1, WIN_IDS,
         16384 * 64 - 1, 16384 * 64,                      # single-block finalise edge
         256 * BLOCK_IDS - 1, 256 * BLOCK_IDS, 257 * BLOCK_IDS - 1, 257 * BLOCK_IDS,
         63 * WIN_IDS - 1, 63 * WIN_IDS]                  # the 64th window
    p += list(range(320, 384))                            # one full word
    return np.unique(np.array([v for v in p if 0 <= v < n], np.int64))


def batch_ids(n, n_random, seed):
    """the planted ids, a third of them again, and random ids with repeats"""
    rng = np.random.default_rng(seed)
    p = planted_ids(n)
    r = rng.integers(0, n, n_random)
    ids = np.concatenate([p, p[::3], r, r[: n_random // 4]])
    return rng.permutation(ids)


# ----------------------------------------------------------------------------- engine rig
class Rig:
    def __init__(self, n, L, T, max_pos, nb, wb, feature_rows=1):
        import _native as nat
        import pinsage_model as pm
        self.nat, self.L, self.T = nat, L, T
        self.eng = pm._Engine(n, 4, 4, 4, L, T, max_pos)
        self.po = nat.EnginePlanOffsets()
        nat.check(nat.lib().pinsage_engine_plan_offsets(self.eng.h, ctypes.byref(self.po)), "plan_offsets")
        self.feats = torch.zeros((feature_rows, 4), dtype=torch.float32, device="cuda")
        self.params = torch.zeros(self.eng.n_params, dtype=torch.float32, device="cuda")
        self.bind(nb, wb)
        self.ws = self.eng.new_workspace(torch.device("cuda"))

    def bind(self, nb, wb):
        self.tab = (nb, wb)
        self.nat.check(self.nat.lib().pinsage_engine_set_tensors(
            self.eng.h, self.nat.ptr(self.feats), 4, self.nat.ptr(nb), self.nat.ptr(wb), nb.shape[1],
            self.nat.ptr(self.params), None, None, None), "set_tensors")

    def run(self, ids, inference=False):
        """frontier (or the inference forward, which needs feature_rows = n) of
        ids on the rig's one workspace; returns the plan read back"""
        lib = self.nat.lib()
        self.ids = torch.from_numpy(np.asarray(ids, np.int64)).cuda()
        fn = lib.pinsage_engine_forward_inference if inference else lib.pinsage_engine_frontier
        self.nat.check(fn(self.eng.h, self.nat.ptr(self.ws), self.nat.ptr(self.ids), len(ids),
                          self.nat.stream_ptr()), "frontier")
        return self.read(len(ids))

    def _i32(self, off, n):
        return self.eng.view(self.ws, int(off), torch.int32, int(n)).cpu().numpy()

    def read(self, n_pos):
        o, po, T = self.eng.off, self.po, self.T
        rS, rN = self.eng.counts(self.ws)  # pinsage_engine_read_counts (synchronises)
        layers = []
        for l in range(self.L):
            cS, cN = int(self._i32(o.count_S[l], 1)[0]), int(self._i32(o.count_N[l], 1)[0])
            assert 0 <= cS <= o.cap_S[l], f"layer {l} count_S: {cS} outside its capacity {o.cap_S[l]}"
            assert 0 <= cN <= o.cap_N[l], f"layer {l} count_N: {cN} outside its capacity {o.cap_N[l]}"
            layers.append({"count_S": cS, "count_N": cN,
                           "S": self._i32(o.members_S[l], cS), "N": self._i32(o.members_N[l], cN),
                           "loc": self._i32(po.loc[l], cS * T), "wloc": self._i32(po.wloc[l], cS * T).view(np.uint32),
                           "self_src": self._i32(po.self_src[l], cS), "q_src": self._i32(po.q_src[l], cN)})
        top = layers[-1]["count_S"]
        return {"layers": layers, "read_counts": (rS, rN), "pos_rank": self._i32(o.pos_rank, n_pos),
                "rank_off": self._i32(po.rank_off, top + 1), "pos_sorted": self._i32(po.pos_sorted, n_pos)}


def _universe_case(n):
    """(T, (nb, wn bits)) of a universe: T = 2 or 3 (T = 1 at n = 1), odd
    universes below 2M with a padded row stride (ld > T), planted rows"""
    if n <= 65:
        T = 1 if n == 1 else 3  # (n = 1: a row of T distinct ids needs T = 1)
        ld = T + (n & 1) if n > 4 else T
        return T, perm_table(n, T, ld, seed=n)
    T = 2 if n > 2_000_000 or n % 3 == 0 else 3
    ld = T + 2 if (n & 1 and n < 2_000_000) else T
    nb, wb = arith_table(n, T, ld, a=1_000_003, seed=n % 1000)
    plant_rows(nb, planted_ids(n), T)
    return T, (nb, wb)


def _universe_ids(n):
    """the batch of a universe: 100 positions naming every id up to 65 ids
    (every set is then the whole universe), else the planted ids and 100 random"""
    if n <= 65:
        return np.concatenate([np.arange(n), np.random.default_rng(n).integers(0, n, 100 - n)])
    return batch_ids(n, 100, seed=n % 977)


# ----------------------------------------------------------------------------- universes
UNIVERSES = [1, 63, 64, 65,               # one word and the word edge
             65_536, 65_537,              # 1024 words: per 1 -> 2, one marking block
             524_288, 524_289,            # whole-bitmap LDS -> one window (in-launch finalise)
             1_048_576, 1_048_577,        # in-launch finalise (per 16) -> multi-block scan / top set
             1_308_672, 1_308_673,        # one window -> two
             83_755_008, 83_755_009]      # 64 windows -> global atomics; > 256 scan blocks


@pytest.mark.parametrize("n", UNIVERSES)
def test_plan_matches_numpy_across_universes(n):
    T, tab = _universe_case(n)
    L = 2
    ids = _universe_ids(n)
    max_pos = 128 if n <= 65 else 256
    assert len(ids) <= max_pos
    want = frontier_plan_reference(ids, rows_of(tab, T), L, T)
    if n == 65:  # every set is the whole universe
        assert want["read_counts"] == ([65, 65], [65, 65])
    rig = Rig(n, L, T, max_pos, *tab)
    check_frontier_plan(rig.run(ids), want)


def test_plan_with_several_marking_blocks_on_the_ticket_path():
    """n = 200 000 (3125 words: whole-bitmap LDS marking, per = 4), max_pos =
    2048, T = 3: cap_S T = 6144 at the top layer (2 marking blocks) and 24 576
    at layer 0 (6 blocks), so the last-block ticket decides among several."""
    n, L, T, max_pos = 200_000, 2, 3, 2048
    nb, wb = arith_table(n, T, T + 1, a=7919, seed=3)
    plant_rows(nb, planted_ids(n), T)
    ids = batch_ids(n, 1500, seed=11)
    assert len(ids) <= max_pos
    rig = Rig(n, L, T, max_pos, nb, wb)
    assert rig.eng.off.cap_S[1] * T > 4096 and rig.eng.off.cap_S[0] * T > 4 * 4096
    want = frontier_plan_reference(ids, rows_of((nb, wb), T), L, T)
    assert want["read_counts"][0][0] * T > 4096  # more than one block has work at layer 0
    check_frontier_plan(rig.run(ids), want)


# ----------------------------------------------------------------------------- positions
def _position_ids(pattern, n_pos, n, seed):
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(n_pos, 4321, np.int64)
    if pattern == "distinct":
        return rng.permutation(n)[:n_pos].astype(np.int64)
    return np.minimum(rng.zipf(1.3, n_pos) - 1, n - 1).astype(np.int64)  # heavy-tailed


@pytest.mark.parametrize("pattern", ["equal", "distinct", "heavy"])
@pytest.mark.parametrize("n_pos", [1, 63, 64, 65, 1024, 1025, 16384, 16385])
def test_position_csr(n_pos, pattern):
    n, L, T = 20_000, 1, 2
    tab = arith_table(n, T, T, a=7919, seed=5)
    ids = _position_ids(pattern, n_pos, n, seed=n_pos)
    want = frontier_plan_reference(ids, rows_of(tab, T), L, T)
    got = Rig(n, L, T, n_pos, *tab).run(ids)
    if n_pos > POS_CSR_MAX:  # handed off: the mark, and pos_rank still right (checked below)
        assert int(got["rank_off"][0]) == -1
    check_frontier_plan(got, want)


# ----------------------------------------------------------------------------- workspace reuse
@pytest.mark.parametrize("n", [65_537, 1_048_577])  # in-launch finalise / multi-block regime
def test_workspace_reuse(n):
    """A large frontier, a small one disjoint from it, the first again, then an
    inference forward (no CSR), all on one workspace: every call must zero all
    bitmaps of the previous one and find its tickets reset."""
    L, T, max_pos = 2, 2, 256
    nb, wb = arith_table(n, T, T + 1, a=1_000_003, seed=9)
    plant_rows(nb, planted_ids(n), T)
    small = n // 2 + 1000 + 5 * np.arange(8, dtype=np.int64)  # rows closed under the table
    plant_rows(nb, small, T)
    big = batch_ids(n, 100, seed=21)
    rows = rows_of((nb, wb), T)
    want_big = frontier_plan_reference(big, rows, L, T)
    want_small = frontier_plan_reference(small[[3, 1, 1, 7, 0, 2, 4, 5, 6]], rows, L, T)
    lay = want_big["layers"][0]
    assert not np.intersect1d(np.concatenate([lay["S"], lay["N"]]), small).size  # the sets do not overlap
    assert want_small["read_counts"] == ([8, 8], [8, 8])
    rig = Rig(n, L, T, max_pos, nb, wb, feature_rows=n)
    check_frontier_plan(rig.run(big), want_big)
    check_frontier_plan(rig.run(small[[3, 1, 1, 7, 0, 2, 4, 5, 6]]), want_small)
    check_frontier_plan(rig.run(big), want_big)
    check_frontier_plan(rig.run(small[[3, 1, 1, 7, 0, 2, 4, 5, 6]], inference=True), want_small)


# ----------------------------------------------------------------------------- engine options
def test_per_layer_tables():
    n, L, T, max_pos = 5000, 2, 3, 256
    tabs = [arith_table(n, T, T + l, a=a, seed=s) for l, (a, s) in enumerate([(7919, 1), (104_729, 2), (31, 3)])]
    ids = batch_ids(n, 100, seed=4)
    rig = Rig(n, L, T, max_pos, *tabs[2])
    lib, nat = rig.nat.lib(), rig.nat
    for l in range(L):
        nat.check(lib.pinsage_engine_set_layer_table(rig.eng.h, l, nat.ptr(tabs[l][0]), nat.ptr(tabs[l][1]),
                                                     tabs[l][0].shape[1]), "set_layer_table")
    check_frontier_plan(rig.run(ids), frontier_plan_reference(ids, rows_of([tabs[0], tabs[1]], T), L, T))
    # one layer back on the engine-wide table, then both
    nat.check(lib.pinsage_engine_set_layer_table(rig.eng.h, 1, None, None, 0), "set_layer_table")
    check_frontier_plan(rig.run(ids), frontier_plan_reference(ids, rows_of([tabs[0], tabs[2]], T), L, T))
    nat.check(lib.pinsage_engine_set_layer_table(rig.eng.h, 0, None, None, 0), "set_layer_table")
    check_frontier_plan(rig.run(ids), frontier_plan_reference(ids, rows_of(tabs[2], T), L, T))


@pytest.mark.parametrize("n_x", [0, 1, 37])
@pytest.mark.parametrize("n", [5000, 1_048_577])  # one-block top set / multi-kernel top set
def test_virtual_nodes_join_the_top_set(n, n_x):
    """pinsage_engine_set_fly: x0 .. x0 + *n_x - 1 (*n_x in device memory) join
    the top set; their ranks take rank_off entries with no position."""
    L, T, max_pos = 2, 2, 256
    tab = arith_table(n, T, T, a=7919, seed=6)
    x0 = n - 37  # (the largest range ends at n - 1)
    ids = batch_ids(n, 60, seed=8)
    # a few positions name ids of the virtual range (one twice); most virtual ranks get no position
    ids = np.concatenate([ids[ids < x0], [x0 + 3, x0 + 10, x0 + 3]]).astype(np.int64)
    assert len(np.unique(ids)) + 37 <= max_pos
    rig = Rig(n, L, T, max_pos, *tab)
    nat, lib = rig.nat, rig.nat.lib()
    nx_dev = torch.tensor([n_x], dtype=torch.int32, device="cuda")
    xids = torch.zeros(64, dtype=torch.int64, device="cuda")
    nat.check(lib.pinsage_engine_set_fly(rig.eng.h, x0, nat.ptr(nx_dev), nat.ptr(xids), 1, 64), "set_fly")
    rows = rows_of(tab, T)
    want = frontier_plan_reference(ids, rows, L, T, virtual=(x0, n_x))
    if n_x == 37:
        assert (np.diff(want["rank_off"]) == 0).any()  # ranks without a position
    check_frontier_plan(rig.run(ids), want)
    nat.check(lib.pinsage_engine_set_fly(rig.eng.h, 0, None, None, 1, 0), "set_fly")
    check_frontier_plan(rig.run(ids), frontier_plan_reference(ids, rows, L, T))


# ----------------------------------------------------------------------------- API path
@pytest.mark.parametrize("n", [u for u in UNIVERSES if u <= 1_308_673])
def test_api_frontier_step_matches_the_same_reference(n):
    """pinsage_frontier_step + pinsage_frontier_local_idx (torch.ops.pinsage.frontier)
    on the boundary universes: the step from the batch ids is the plan's S_0,
    the step from S_0 is unique(N_0 | S_0), local_idx the ranks in them."""
    import pinsage_ops
    pinsage_ops.load()
    T, tab = _universe_case(n)
    nb = tab[0]
    ids = _universe_ids(n)
    rows = rows_of(tab, T)
    want = frontier_plan_reference(ids, rows, 2, T)
    S0, N0 = want["layers"][0]["S"], want["layers"][0]["N"]
    below = np.unique(np.concatenate([N0, S0]))
    for nodeset, uniq_ref in ((ids, S0), (S0, below)):
        uniq, local = torch.ops.pinsage.frontier(torch.from_numpy(nodeset).cuda(), nb, T)
        assert np.array_equal(uniq.cpu().numpy(), uniq_ref), "frontier step: nodes_out"
        assert np.array_equal(local.cpu().numpy().astype(np.int64),
                              np.searchsorted(uniq_ref, rows(0, nodeset)[0])), "frontier step: local_idx"
