"""Seeded inputs of the loss-step tests (tests/test_gpu_loss_step.py; checked on the CPU by tests/test_loss_step_mirror.py) -- TEST
INFRASTRUCTURE.  Shapes are the smallest at which each path of csrc/loss.hip can break, nothing is at workload size:
  d   16, 48 (ng = 1, masked) | 64, 128, 256 (exact; both finishes) | 192, 320 (masked ng = 4 / 8) | 512 (ng = 8, no held i tile)
      | 576, 1024 (nz = 2, masked and exact)
  b   1, 15, 16, 17, 63, 64, 65, 333 (the 16-row tile, the 64 rows of a workgroup's 4 waves) | 1040 (65 tiles: js reaches its cap of 16)
  loss_wgs 64 / 256 / 4096: js = 1 / 4 / 16 at b = 1040, 4 / 6 / 6 at b = 333

Every case passes loss_step_mirror.pair_guard with ZERO unsafe pairs: its seed is the first of 0, 1, 2, ... for which no pair's fp32 dot
product can land on the other side of zero.  With mixed-sign Gaussian rows (the x[:, 0] += 1 recipe of test_loss_fwd_bwd) the chance
that a pair falls inside the band grows with b^2 d, so the search ends quickly up to b = 333 at d <= 128 and at the small batches of
the wide rows; at b = 1040 (540,280 pairs; ~20 expected inside the band) no seed passes, and those cases use the regime "signed":
rows with positive entries (squares of Gaussians) times a random sign per row: every product of a pair has the pair's sign, so
|S| = sum_k |e_ik e_jk| and the guard holds whatever the seed, with both signs and both sides of beta present."""
import functools

import numpy as np

import loss_step_mirror as M

ALPHA = 1.7
C = 0.4
REGIMES = {            # name -> beta
    "recipe": 0.25,    # x[:, 0] += 1: mostly positive similarities, some negative
    "below": 0.9,      # rows of norm 0.9: every similarity, the diagonal included, is below beta
    "beta0": 0.0,
    "negbeta": -0.3,
    "orth": 0.25,      # the first rows are signed unit vectors on distinct features: S exactly 0 among them
    "signed": 0.25,    # rows of squares times a sign per row: |S| spreads around 1 / 3, on both sides of beta
}

# every d at two or three batch sizes, every b at d in {64, 128}, b = 1040 at d in {64, 128} only
SHAPES = ([(d, b) for d in (64, 128) for b in (1, 15, 16, 17, 63, 64, 65, 333)]
          + [(16, 17), (16, 65), (48, 15), (48, 64), (256, 16), (256, 63), (256, 65), (192, 17), (192, 65), (320, 1), (320, 63),
             (512, 16), (512, 65), (576, 17), (576, 65), (1024, 15), (1024, 64)])
# (regime, d, b, loss_wgs)
STEP_CASES = ([("recipe", d, b, 256) for d, b in SHAPES]
              + [("signed", d, 1040, w) for d in (64, 128) for w in (64, 256, 4096)]
              + [("recipe", 64, 333, 64), ("recipe", 128, 333, 4096), ("recipe", 576, 65, 64), ("recipe", 320, 63, 4096)]
              + [(r, d, b, 256) for r in ("below", "beta0", "negbeta", "orth", "signed") for d, b in ((48, 64), (128, 65), (192, 17), (576, 65))])
# the finish with the input gradient (d in {64, 128, 256})
WEIGHT_CASES = ([("recipe", d, b, 256) for d in (64, 128, 256) for b in (1, 17, 65)] + [("recipe", 64, 333, 64), ("recipe", 128, 333, 256)]
                + [("signed", 256, 333, 256), ("orth", 128, 64, 256), ("signed", 64, 1040, 4096), ("signed", 128, 1040, 64)])
REFUSED_WIDTHS = (192, 512, 1024)
# (regime, d, b, parts); b = 17 with 8 parts leaves six ranks without a tile
SLAB_CASES = [("signed" if b == 1040 else "recipe", d, b, parts) for parts in (2, 3, 8) for b in (17, 65, 333, 1040) for d in (64, 128, 192)
              if not (b == 1040 and d == 192)]
REPEAT_CASES = [("recipe", 64, 65, 256), ("recipe", 192, 17, 256), ("recipe", 128, 333, 64)]
GATHER_SHAPES = [(b, d) for b in (1, 17, 333) for d in (16, 128, 320)]


def _rows(regime, d, n, rng):
    """x [n][d] (fp64): the matrix whose normalised rows are the embeddings"""
    x = rng.randn(n, d)
    if regime == "signed":
        return x * x * rng.choice([-1.0, 1.0], size=(n, 1))
    x[:, 0] += 1.0
    if regime == "orth":
        m = min(n // 2, d)
        x[:m] = 0.0
        x[np.arange(m), rng.permutation(d)[:m]] = rng.choice([-1.0, 1.0], size=m) * rng.uniform(0.5, 2.0, size=m)
    return x


def _build(regime, d, b, seed):
    rng = np.random.RandomState((seed * 1000003 + d * 4099 + b) % (2 ** 31))
    n = b + 7
    x = _rows(regime, d, n, rng)
    den = np.sqrt((x ** 2).sum(1))
    e = x / den[:, None] * (0.9 if regime == "below" else 1.0)
    rows = rng.permutation(n)[:b].astype(np.int32)
    if regime == "orth":                      # about half of the batch comes from the orthogonal block
        m = min(n // 2, d)
        k = min(m, max(b // 2, 1))
        rows = np.concatenate([rng.permutation(m)[:k], m + rng.permutation(n - m)[:b - k]])[rng.permutation(b)].astype(np.int32)
    p = rng.randn(n, d)
    keep = (rng.rand(b) > 1.0 / 3.0).astype(np.float32)
    keep[0] = keep[-1] = 0.0                  # the first and the last member, and one whole 16-row tile
    if b >= 32:
        t = (b // 16) // 2
        keep[16 * t:16 * t + 16] = 0.0
    if b > 2:
        keep[1] = 1.0
    c = dict(regime=regime, d=d, b=b, n=n, seed=seed, beta=REGIMES[regime], alpha=ALPHA, c=C,
             e=e.astype(np.float32), inv_den=(1.0 / den).astype(np.float32), p=p.astype(np.float32), rows=rows, keep=keep,
             w1t=(rng.randn(d, d) / np.sqrt(d)).astype(np.float32), w2t=(rng.randn(d, d) / np.sqrt(d)).astype(np.float32))
    c["e_b"] = c["e"][rows]
    # the per-member form of a shard's gathered batch: p / inv_den of b rows, in batch order
    c["p_b"], c["inv_b"] = c["p"][rows], c["inv_den"][rows]
    return c


@functools.lru_cache(maxsize=None)
def case(regime, d, b):
    """the inputs of (regime, d, b): the first seed whose batch has no unsafe pair.  Arrays are shared between tests: read only"""
    for seed in range(400):
        c = _build(regime, d, b, seed)
        if M.pair_guard(c["e_b"]) == 0:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            return c
    raise AssertionError(f"no seed below 400 gives ({regime}, d={d}, b={b}) a batch without unsafe pairs")


@functools.lru_cache(maxsize=None)
def reference(regime, d, b, form, weights=False, dgrad_all=False):
    """the fp64 mirror of gss_loss_step on case(regime, d, b); form: "ids" (rows = ids, no keep) or "member" (rows NULL, keep)"""
    c = case(regime, d, b)
    w = dict(w1t=c["w1t"], w2t=c["w2t"], dgrad_all=dgrad_all) if weights else {}
    if form == "ids":
        return M.step(c["e_b"], c["beta"], c["alpha"], c["inv_den"], c["p"], c["c"], rows=c["rows"], **w)
    return M.step(c["e_b"], c["beta"], c["alpha"], c["inv_b"], c["p_b"], c["c"], keep=c["keep"], **w)


def repeated(regime, d, b):
    """a batch with repeated ids: every third member repeats the one before it (loss and dE only; the finish needs distinct ids)"""
    c = case(regime, d, b)
    rows = c["rows"].copy()
    rows[2::3] = rows[1::3][:len(rows[2::3])]
    return c, rows
