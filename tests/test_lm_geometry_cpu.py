"""The block schedule of the LM pass (csrc/hedge_narrow.h NarrowPairBody::sched)
as rphedge.engine.lm_pass_blocks states it on the host: every 128-path block
of a batch is taken by exactly one wave, in every regime (cyclic, split,
contiguous leaves); and the launch geometry of every case of
tests/test_gpu_lm_geometry.py (CASES below) enters the regime its row names -
path schedule, packet tree and Gram tree of k_lm_reduce - so a later change of
a cap moves no case to another regime unnoticed."""
import numpy as np
import pytest

# ---------------------------------------------------------------------------
# The launch geometries of tests/test_gpu_lm_geometry.py.  ``over``: LmDesc
# fields overridden after the descriptor is built (the buffers are sized for
# the natural, larger geometry); ``gram_k``: the Gram overridden to the prefix
# of 64 k paths; ``overlap``: Gram-only workgroups after the path grid
# (gram_base = num_wgs).  ``expect``: (path regime, blocks per Gram wave or
# None, packet tree, Gram tree, path workgroups, Gram workgroups).
# ---------------------------------------------------------------------------
S_1820, S_1811, S_2820, S_3820, S_5860 = (1, 8, 2, 0), (1, 8, 1, 1), (2, 8, 2, 0), (3, 8, 2, 0), (5, 8, 6, 0)
WPS = {S_1820: 2, S_2820: 2, S_1811: 1, S_3820: 1, S_5860: 1}  # native.lm_pass_wps (the GPU module asserts it)


def _case(name, n, shapes, expect, gram_paths=2048, leaf_paths=-1, over=None, gram_k=None, overlap=False, seed=0):
    return dict(name=name, n=n, shapes=shapes, expect=expect, gram_paths=gram_paths, leaf_paths=leaf_paths,
                over=dict(over or {}), gram_k=gram_k, overlap=overlap, seed=seed)


NAT = [S_1820, S_1811, S_5860]
SPL = [S_1820, S_3820, S_5860]
LEAF = [S_1820, S_3820]
CASES = [
    # natural geometry (cyclic: per = 0 at one workgroup per 256 paths)
    _case("nat256", 256, NAT, ("cyclic", None, "one", "thread", 1, 4), gram_paths=256),
    _case("nat832", 832, NAT, ("cyclic", None, "one", "thread", 3, 4), gram_paths=256),
    _case("nat4096", 4096, NAT, ("cyclic", None, "one", "thread", 16, 16), gram_paths=1024),
    _case("nat4416", 4416, NAT, ("cyclic", None, "r32", "lds", 17, 17), gram_paths=1088),
    _case("nat8192", 8192, NAT, ("cyclic", None, "r32", "lds", 32, 32), gram_paths=2048),
    _case("nat8512", 8512, NAT, ("cyclic", None, "r4", "lds", 33, 32), gram_paths=2048),
    # (data seed 6: with _setup's seed 0 the last 64 of the 65,856 paths hold 9.5e-4 and 9.9e-4 of the fp64
    # loss sum on the two nets - below the 1e-3 at which a dropped half block must fail the loss check, since
    # 64 / 65856 = 9.7e-4 on average; seed 6 is the first of 0, 1, ... whose tail passes on both: 1.009e-3,
    # 1.028e-3.  Chosen from the fp64 reference alone; the GPU test asserts the condition itself)
    _case("nat65856", 65856, [S_1820, S_2820], ("cyclic", None, "r4x2", "lds", 257, 64), gram_paths=4096, seed=6),
    # the split schedule (the production one: euro30 at 2^20 paths has per = 4, gram_skip = 3, gb = 1)
    _case("split8192", 8192, SPL, ("split", 1, "one", "thread", 4, 1), over=dict(num_wgs=4, gram_skip=3), gram_k=1),
    _case("split5120", 5120, SPL, ("split", 2, "one", "thread", 2, 1), over=dict(num_wgs=2, gram_skip=3), gram_k=1),
    _case("split5184", 5184, SPL, ("split", 2, "one", "thread", 2, 1), over=dict(num_wgs=2, gram_skip=3), gram_k=1),
    _case("split10304s3", 10304, SPL, ("split", 2, "one", "thread", 4, 2), over=dict(num_wgs=4, gram_skip=3), gram_k=2),
    _case("split10304s1", 10304, SPL, ("split", 4, "one", "thread", 4, 2), over=dict(num_wgs=4, gram_skip=1), gram_k=2),
    _case("split2048", 2048, SPL, ("split", 0, "one", "thread", 2, 1), over=dict(num_wgs=2, gram_skip=3), gram_k=1),
    # contiguous leaves, the Gram tiles in the first workgroups of the grid and after the path grid
    _case("leaf5184", 5184, LEAF, ("leaf", None, "one", "thread", 3, 16), gram_paths=1024,
          over=dict(num_wgs=3, leaf_blocks=4)),
    _case("leaf5184ov", 5184, LEAF, ("leaf", None, "one", "thread", 3, 16), gram_paths=1024,
          over=dict(num_wgs=3, leaf_blocks=4), overlap=True),
    _case("leaf4416", 4416, LEAF, ("leaf", None, "r32", "lds", 17, 17), gram_paths=1088, leaf_paths=0),
    _case("leaf4416ov", 4416, LEAF, ("leaf", None, "r32", "lds", 17, 17), gram_paths=1088, leaf_paths=0, overlap=True),
]
CASE = {c["name"]: c for c in CASES}
# blocks per wave the issue's table gives (5184: the remainder lands on wave 4, the first non-Gram wave)
WAVE_BLOCKS = {"split5120": [2, 2, 2, 2, 8, 8, 8, 8], "split5184": [2, 2, 2, 2, 9, 8, 8, 8],
               "leaf5184": [4] * 10 + [1, 0], "leaf5184ov": [4] * 10 + [1, 0],
               "leaf4416": [1] * 35 + [0] * 33, "leaf4416ov": [1] * 35 + [0] * 33}


def case_geometry(case, wps):
    """The LmDesc geometry HipBackend builds for ``case`` (one rank) with its
    overrides applied, computed on the host alone."""
    from rphedge.engine import gram_subsample, lm_pass_schedule
    from rphedge.ops import layout as L

    n = case["n"]
    nw, leaf = lm_pass_schedule(n, case["leaf_paths"], wps)
    ns, blk, stride = gram_subsample(n, case["gram_paths"])
    g = dict(num_wgs=nw, leaf_blocks=leaf, gram_wgs=ns // L.LM_TILE, gram_blk=blk, gram_blk_stride=stride,
             inv_ns=1.0 / ns, gram_skip=3)
    g["natural_wgs"], g["natural_gram_wgs"] = nw, g["gram_wgs"]
    g.update(case["over"])
    if case["gram_k"] is not None:
        k = case["gram_k"]
        g.update(gram_wgs=k, gram_blk=64 * k, gram_blk_stride=n, inv_ns=1.0 / (64 * k))
    g["gram_base"] = g["num_wgs"] if case["overlap"] else 0
    return g


def case_blocks(case, wps):
    """(regime, blocks per wave) of the case's pass 0, as k_lm_pass calls the
    schedule: no Gram workgroup among the path workgroups with gram_base > 0."""
    from rphedge.engine import lm_pass_blocks

    g = case_geometry(case, wps)
    return lm_pass_blocks(case["n"], g["num_wgs"], 0 if g["gram_base"] > 0 else g["gram_wgs"], g["gram_skip"],
                          g["leaf_blocks"])


def wave_paths(blocks, n):
    """Paths of a wave's blocks, masked at the end of the batch."""
    return sum(max(0, min(128, n - 128 * b)) for b in blocks)


def _exactly_once(blocks, nblk):
    flat = np.fromiter((b for w in blocks for b in w), dtype=np.int64)
    return flat.size == nblk and (nblk == 0 or (flat.min() >= 0 and flat.max() < nblk)) and \
        np.array_equal(np.bincount(flat, minlength=nblk), np.ones(nblk, np.int64))


BATCHES = list(range(64, 20000, 64)) + [1 << 15, 1 << 17, (1 << 17) + 64]
NUM_WGS = [1, 2, 3, 4, 5, 16, 17, 32, 33]
GRAM_WGS = [1, 2, 4, 7, 64]
GRAM_SKIP = [0, 1, 3]


def test_every_block_is_taken_exactly_once():
    """Cyclic and split schedules over the sweep: every block of [0, ceil(batch
    / 128)) belongs to exactly one wave; in the split regime every wave of the
    Gram workgroups takes max(per - gram_skip, 0) blocks; every regime occurs."""
    from rphedge.engine import lm_pass_blocks

    seen, bad = {}, []
    for batch in BATCHES:
        nblk = (batch + 127) // 128
        for nw in NUM_WGS:
            for gw in GRAM_WGS:
                for skip in GRAM_SKIP:
                    regime, blocks = lm_pass_blocks(batch, nw, gw, skip)
                    ok = len(blocks) == 4 * nw and _exactly_once(blocks, nblk)
                    per = nblk // (4 * nw)
                    split = skip > 0 and gw < nw and per > 0
                    ok = ok and regime == ("split" if split else "cyclic")
                    if split:
                        gb = max(per - skip, 0)
                        ok = ok and all(len(blocks[w]) == gb for w in range(4 * gw))
                        seen["gb>0" if gb else "gb=0"] = seen.get("gb>0" if gb else "gb=0", 0) + 1
                    seen[regime] = seen.get(regime, 0) + 1
                    if not ok:
                        bad.append((batch, nw, gw, skip))
    assert not bad, (len(bad), bad[:10])
    assert seen["cyclic"] > 1000 and seen["gb>0"] > 1000 and seen["gb=0"] > 1000, seen


def test_every_block_is_taken_exactly_once_by_a_leaf():
    """Contiguous leaves the launcher accepts (leaf_blocks x 512 x num_wgs >=
    batch): exactly once, in ascending order along the waves; a leaf schedule
    that does not cover the batch leaves blocks out (what the launcher refuses)."""
    from rphedge.engine import lm_pass_blocks

    bad = []
    for batch in BATCHES:
        nblk = (batch + 127) // 128
        for nw in NUM_WGS:
            lb0 = -(-batch // (512 * nw))
            for lb in (lb0, lb0 + 1, 2 * lb0):
                assert lb * 512 * nw >= batch
                regime, blocks = lm_pass_blocks(batch, nw, 7, 3, lb)
                flat = [b for w in blocks for b in w]
                if regime != "leaf" or len(blocks) != 4 * nw or flat != list(range(nblk)) or \
                        any(len(w) > lb for w in blocks):
                    bad.append((batch, nw, lb))
            if lb0 > 1:
                _, blocks = lm_pass_blocks(batch, nw, 7, 3, lb0 - 1)
                assert sum(len(w) for w in blocks) < nblk
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("name", list(CASE))
def test_gpu_case_enters_its_regime(name):
    """The regime table of the GPU cases: path schedule (and the blocks of a
    Gram wave), packet tree, Gram tree, path and Gram workgroups - for every
    shape of the case (R = 128 and 256, one or two pass workgroups per CU)."""
    from rphedge.engine import lm_pass_blocks, lm_reduce_trees

    case = CASE[name]
    regime, gb, pk, gram, nw, gw = case["expect"]
    for shape in case["shapes"]:
        g = case_geometry(case, WPS[shape])
        got, blocks = case_blocks(case, WPS[shape])
        assert (got, g["num_wgs"], g["gram_wgs"]) == (regime, nw, gw), shape
        assert g["num_wgs"] <= g["natural_wgs"] and g["gram_wgs"] <= g["natural_gram_wgs"]  # inside the buffers
        assert _exactly_once(blocks, (case["n"] + 127) // 128)
        if regime == "split":
            assert all(len(blocks[w]) == gb for w in range(4 * gw))
            assert sum(len(w) for w in blocks[4 * gw:]) == (case["n"] + 127) // 128 - 4 * gw * gb
        for R in (128, 256):
            assert lm_reduce_trees(R, g["num_wgs"], g["gram_wgs"]) == (pk, gram)
        if name in WAVE_BLOCKS:
            assert [len(w) for w in blocks] == WAVE_BLOCKS[name]
        if regime != "cyclic":
            # the GPU module's per-row path counts tell this schedule from a fallback to the cyclic one
            _, cyc = lm_pass_blocks(case["n"], g["num_wgs"], 0, 0)
            rows = [[sum(wave_paths(b[4 * w + k], case["n"]) for k in range(4)) for w in range(nw)] for b in (blocks, cyc)]
            # (leaves of one block on more waves than blocks ARE the cyclic schedule: leaf4416)
            assert (rows[0] != rows[1]) == (max(len(w) for w in blocks) > 1), name
            assert sum(rows[0]) == sum(rows[1]) == case["n"]
        # the last Gram slot stays inside the shard (the launcher's own condition)
        ns = 64 * g["gram_wgs"]
        assert ((ns - 1) // g["gram_blk"]) * g["gram_blk_stride"] + (ns - 1) % g["gram_blk"] < case["n"]


def test_gpu_cases_cover_every_regime():
    """Every regime the kernels' geometry tables name is entered by a case."""
    from rphedge.engine.lm_geometry import LM_PK_C_MAX, LM_TPE_MAX

    exp = [c["expect"] for c in CASES]
    assert {e[2] for e in exp} == {"one", "r32", "r4", "r4x2"} and {e[3] for e in exp} == {"thread", "lds"}
    assert {e[0] for e in exp} == {"cyclic", "split", "leaf"}
    assert {e[1] for e in exp if e[0] == "split"} >= {0, 1, 2, 4}
    nws = {e[4] for e in exp}
    # both sides of every row-count threshold of the packet trees, and of the Gram tree's
    assert {LM_TPE_MAX, LM_TPE_MAX + 1, LM_PK_C_MAX, LM_PK_C_MAX + 1, 257} <= nws and 1 in nws
    assert {LM_TPE_MAX, LM_TPE_MAX + 1} <= {e[5] for e in exp}
    # ragged batches (a last block half past the end) in every path regime; masked rows (no power of two)
    assert {c["expect"][0] for c in CASES if c["n"] % 128 == 64} == {"cyclic", "split", "leaf"}
    assert any(nw & (nw - 1) for nw in nws)
    # a split remainder that falls to a non-Gram wave, a clipped leaf and an empty one
    assert WAVE_BLOCKS["split5184"][4] == 9 and 1 in WAVE_BLOCKS["leaf5184"] and 0 in WAVE_BLOCKS["leaf5184"]
    # the production ratios (euro30 at 2^20 paths: 512 workgroups, 64 Gram workgroups, gram_skip 3)
    from rphedge.engine import lm_pass_blocks

    regime, blocks = lm_pass_blocks(1 << 20, 512, 64, 3)
    assert regime == "split" and (1 << 20) // 128 // 2048 == 4 and {len(w) for w in blocks[:256]} == {1}
    assert _exactly_once(blocks, 8192)
