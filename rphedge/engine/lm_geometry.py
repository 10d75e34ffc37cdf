"""Integer geometry of the Levenberg-Marquardt launches (mirrors csrc/hedge_lm.hip): workgroup counts, path
schedules, the Gram subsample, the reduced block's layout.  Shared by both backends, the driver and the tests."""
from __future__ import annotations

import numpy as np

from ..ops import layout as L

GRAM_BLOCKS = 8  # global blocks of the LM Gram subsample (the largest single-node world size)


def _lm_bias_index(spec, t) -> int:
    """LmDesc.bias_index: the bond holding's output bias (the last parameter of
    a free-head net), -1 for the complement head or with lm_bias_fix off."""
    return spec.nparams - 1 if (t.lm_bias_fix and spec.head == L.HEAD_FREE) else -1


def lm_out_nu(spec) -> int:
    """Output-layer parameters of a net (csrc/hedge_narrow.h NarrowPairBody::NU):
    free head H x NO + NO, complement head H + 1."""
    return spec.hidden * spec.nout + spec.nout if spec.head == L.HEAD_FREE else spec.hidden + 1


def lm_out_gram(spec) -> bool:
    """The LM pass can build the full-batch output-layer Gram matrix on the
    matrix cores (NarrowPairBody OG: at most LM_OG_MAX output parameters)."""
    return spec.hidden == 8 and lm_out_nu(spec) <= L.LM_OG_MAX


def lm_og_wgs(spec) -> int:
    """Output-Gram workgroups of k_lm_reduce (64 packed entries each)."""
    nu = lm_out_nu(spec)
    npk = nu * (nu + 1) // 2
    epw = 16 if npk <= 512 else 64  # (csrc/hedge_lm.hip lm_og_epw)
    return (npk + epw - 1) // epw if nu <= L.LM_OG_MAX else 0


def _lm_out_n(spec, t) -> int:
    """LmDesc.out_n: output-layer parameters of the final exact Newton step
    with the full-batch output Gram (TrainConfig.lm_out_fix), 0 = the bias
    step alone."""
    return lm_out_nu(spec) if (t.lm_out_fix and lm_out_gram(spec)) else 0


def gram_subsample(n_total: int, lm_gram_paths: int) -> tuple[int, int, int]:
    """(ns, blk, stride) of the LM Gram subsample of a ``n_total``-path run: the
    first ``blk`` paths of each of ns / blk aligned global blocks of ``stride``
    paths (GRAM_BLOCKS blocks where the sizes allow: aligned prefixes of a
    Sobol sequence are nets; a strided subset is not).  The same global paths
    at every world size: every rank simulates them (index-addressable Sobol /
    Philox) and builds the identical Gram matrix, so the data-parallel exchange
    carries only the gradient region [g | stats | out-means]."""
    n_total = int(n_total)
    ns = max(L.LM_TILE, min(int(lm_gram_paths), n_total) // L.LM_TILE * L.LM_TILE)
    nb = GRAM_BLOCKS
    while nb > 1 and (ns % (L.LM_TILE * nb) or n_total % nb):
        nb //= 2
    return ns, ns // nb, n_total // nb


def lm_pass_wgs(n_local: int, wps: int = 1) -> int:
    """Workgroups of the LM pass kernel (HipBackend._lm_buffers; the torch
    oracle derives its Gram subsample from the same number): ``wps`` per CU
    (256 CUs; 2 for the nets whose plain pass body fits twice on a CU,
    native.lm_pass_wps), at most one per 256 local paths."""
    return int(max(1, min(256 * max(1, min(int(wps), L.LM_PASS_WGS_MAX // 256)), n_local // 256)))


def lm_pass_schedule(n_local: int, leaf_paths: int = 0, wps: int = 1) -> tuple[int, int]:
    """(pass workgroups, leaf blocks) of an LM pass over ``n_local`` paths
    (TrainConfig.lm_leaf_paths): auto (0) = lm_pass_wgs workgroups, the shard
    split into 4 x that many contiguous leaves; > 0 = leaves of that many
    paths (the workgroups to cover them, at most 256 x wps); < 0 = the cyclic
    schedule (leaf 0)."""
    nw = lm_pass_wgs(n_local, wps)
    nmax = lm_pass_wgs(1 << 40, wps)
    nblk = (int(n_local) + 127) // 128
    if leaf_paths < 0:
        return nw, 0
    if leaf_paths > 0:
        if leaf_paths % 128:
            raise ValueError(f"lm_leaf_paths must be a multiple of 128, got {leaf_paths}")
        # the world-invariance contract (a rank's rows form a complete subtree of
        # the one-rank contiguous-halves tree): whole leaves per shard and a
        # power-of-two number of pass workgroups per rank
        if int(n_local) % leaf_paths:
            raise ValueError(f"lm_leaf_paths {leaf_paths} does not divide the {n_local}-path shard")
        lb = leaf_paths // 128
        nw = int(min(nmax, max(1, -(-nblk // (4 * lb)))))
        if 4 * nw * lb < nblk:
            raise ValueError(f"{leaf_paths}-path leaves need more than {nmax} pass workgroups for {n_local} paths")
        if nw & (nw - 1):
            raise ValueError(f"lm_leaf_paths {leaf_paths} gives {nw} pass workgroups for {n_local} paths; world "
                             "invariance needs a power of two (choose a power-of-two shard and leaf size)")
        return nw, lb
    return nw, int(-(-nblk // (4 * nw)))


def lm_pass_blocks(batch: int, num_wgs: int, gram_wgs: int, gram_skip: int, leaf_blocks: int = 0):
    """(regime, blocks): the 128-path blocks of every wave of an LM pass over
    ``batch`` paths (csrc/hedge_narrow.h NarrowPairBody::sched, line by line);
    ``blocks[w]`` lists the blocks of wave ``w`` = 4 x workgroup + wave, in the
    order the wave runs them.  ``gram_wgs`` is what k_lm_pass hands the
    schedule: 0 with Gram-only workgroups after the path grid (LmDesc.gram_base
    > 0) and in a final evaluation.  Regimes: "leaf" (contiguous leaves),
    "cyclic", and "split" - the waves of the Gram workgroups take gram_skip
    blocks fewer than an even split (``gb`` each, possibly none), the others
    share the rest."""
    nblk = (int(batch) + 127) // 128
    TW = int(num_wgs) * 4
    if leaf_blocks > 0:
        out = []
        for w in range(TW):
            b0 = w * leaf_blocks
            b1 = b0 + leaf_blocks
            out.append(list(range(b0, b1 if b1 < nblk else nblk)))
        return "leaf", out
    GW = (gram_wgs if gram_wgs < num_wgs else num_wgs) * 4
    per = nblk // TW
    if gram_skip <= 0 or GW >= TW or per <= 0:
        return "cyclic", [list(range(w, nblk, TW)) for w in range(TW)]
    gb = per - gram_skip if per > gram_skip else 0
    out = []
    for w in range(TW):
        if w < GW:
            out.append(list(range(w, GW * gb, GW)))
        else:
            out.append(list(range(GW * gb + (w - GW), nblk, TW - GW)))
    # (no Gram workgroup among the path workgroups: the second branch alone, which is the cyclic schedule)
    return ("split" if GW > 0 else "cyclic"), out


LM_TPE_MAX = 16   # csrc/hedge_lm.hip: Gram slabs / packet rows up to which k_lm_reduce sums an entry in one thread
LM_PK_C_MAX = 32  # packet rows up to which a reduce workgroup takes 32 entries


def lm_gram_red_wgs(ng: int, gram_wgs: int) -> int:
    """Gram workgroups of k_lm_reduce over ``ng`` Gram entries (csrc/hedge_lm.hip
    lm_gram_red_wgs): 1,024 entries each up to LM_TPE_MAX slabs, else 64."""
    return ng // 1024 if gram_wgs <= LM_TPE_MAX else ng // 64


def lm_pk_red_wgs(R: int, num_wgs: int, dp_fused: int = 0) -> int:
    """Packet workgroups of k_lm_reduce (csrc/hedge_lm.hip lm_pk_red_wgs)."""
    if dp_fused:
        return R // 4
    return 1 if num_wgs <= LM_TPE_MAX else R // 32 if num_wgs <= LM_PK_C_MAX else R // 4


def lm_reduce_trees(R: int, num_wgs: int, gram_wgs: int) -> tuple[str, str]:
    """(packet tree, Gram tree) k_lm_reduce runs without the fused exchange:
    packet "one" (one workgroup, thread = entry), "r32" (32 entries per
    workgroup), "r4" (4 entries, up to 256 rows) or "r4x2" (up to 512 rows, one
    level deeper); Gram "thread" (thread = entry) or "lds"."""
    npw = lm_pk_red_wgs(R, num_wgs)
    pk = "one" if npw == 1 else "r32" if npw == R // 32 else "r4" if num_wgs <= 256 else "r4x2"
    return pk, ("thread" if lm_gram_red_wgs(1024, gram_wgs) == 1 else "lds")


def lm_tpack_len(P: int, nblk: int) -> int:
    """Doubles of the solve's tile-store image of the Gram that k_lm_reduce
    writes after the 32 x 32 blocks (csrc/hedge_lm.hip LmTPack: nets with up
    to 48 tiles whose blocks and image fit the Gram region), else 0.  A Gram
    all-reduce over the ranks carries it with the blocks."""
    nt = (P + 1 + 15) // 16
    ntile = nt * (nt + 1) // 2
    nx = (P + 15) // 16 - 1 if ntile <= 48 else 0
    ln = ntile * 256
    return ln if nx > 0 and nblk * 1024 + ln <= L.LM_GBLK_MAX else 0


def lm_tpack_image(blocks, P: int, nblk: int):
    """The tile-store image k_lm_reduce writes at red[nblk * 1024:] (strictly
    lower Gram entries x2 at their csrc/lm_chol.h tile-store offsets) from the
    32 x 32 blocks red[:nblk * 1024], for code that builds a reduced block on
    the host (tests); None when the net has no image (lm_tpack_len 0)."""
    ln = lm_tpack_len(P, nblk)
    if ln == 0:
        return None
    nbg, nt = (P + 31) // 32, (P + 1 + 15) // 16
    e = np.arange(nblk * 1024)
    b, f = e >> 10, e & 1023
    starts = np.cumsum([0] + [nbg - m for m in range(nbg)])
    mb = np.searchsorted(starts, b, side="right") - 1
    nb = mb + (b - starts[mb])
    q, h = f >> 6, (f >> 5) & 1
    lo = 32 * mb + (q & 3) + 4 * h + 8 * (q >> 2)
    hi = 32 * nb + (f & 31)
    ok = (lo < hi) & (hi < P)
    ib, jb, r, c = hi >> 4, lo >> 4, hi & 15, lo & 15
    t = jb * nt - jb * (jb - 1) // 2 + (ib - jb)
    off = t * 256 + r * 16 + (c ^ ((r >> 1) << 1))
    img = np.zeros(ln)
    img[off[ok]] = 2.0 * np.asarray(blocks, dtype=np.float64)[:nblk * 1024][ok]
    return img


def lm_gram_geometry(n_local: int, ns_local: int, world: int) -> tuple[int, int]:
    """(gram_blk, gram_blk_stride) of the LM Gram subsample (LmDesc) on one of
    ``world`` ranks: the first paths of this rank's GRAM_BLOCKS / world aligned
    blocks (gram_subsample: the same global paths at world size 1, 2, 4, 8)."""
    bpr = max(1, GRAM_BLOCKS // max(int(world), 1))   # blocks per rank
    while bpr > 1 and (ns_local % bpr or n_local % bpr):
        bpr //= 2
    return max(1, ns_local // bpr), max(1, n_local // bpr)


def lm_shard_gram_wgs(n_local: int, lm_gram_paths: int, world: int, pass_wgs: int) -> int:
    """Gram workgroups (64-path tiles) of a subsample read from the shard: this
    rank's lm_gram_paths / world paths, at most one tile per pass workgroup."""
    ns_local = max(L.LM_TILE, min(int(lm_gram_paths) // world, int(n_local)))
    return int(max(1, min(ns_local // L.LM_TILE, pass_wgs)))


def lm_explore_nsub(fcfg, n_local: int) -> int:
    """Paths of a multi-start exploration: the global prefix (a multiple of 256: one pass workgroup per 256 paths)."""
    have = int(fcfg.lm_explore_data.target.numel()) if fcfg.lm_explore_data is not None else int(n_local)
    want = int(fcfg.lm_explore_paths) if int(fcfg.lm_explore_paths) > 0 else have
    return int(max(256, min(have, want) // 256 * 256))
