"""GPU: the three nulls brought to the host in pieces (_nulls.chunked_null behind classes.null_sums, mantel.null_cross_sums and
enrich.null_scores) equal the single call bit for bit.  The raw ops' own tests cut a call through `first`; this cuts through the byte
budget, unevenly (7 samples as 3 + 3 + 1), at sizes one past a wave: n = 65 rows padded to 128, M = 130 places with sets of 1, 64 and 65."""
import numpy as np
import pytest
import torch

from gcn_drug_repurposing_amd import _nulls as N
from gcn_drug_repurposing_amd import classes as K
from gcn_drug_repurposing_amd import enrich as E
from gcn_drug_repurposing_amd import mantel as MT

pytestmark = pytest.mark.gpu

SAMPLES, SEED = 7, 2 ** 63 + 5


def symmetric(n, seed, signed):
    rng = np.random.RandomState(seed)
    h = np.triu(rng.randn(n, n) if signed else rng.rand(n, n), 1)
    return torch.from_numpy(h + h.T).cuda()


def in_pieces(monkeypatch, module, op, bytes_per_sample, null):
    """null() under a budget of three samples and a half -> (its result, the (count, first) of the calls of module.op it made)"""
    issued, raw = [], getattr(module, op)

    def recorded(*args, **kw):
        issued.append((args[-3], args[-1]))      # (..., count, seed, first) in all three
        return raw(*args, **kw)
    with monkeypatch.context() as m:
        m.setattr(N, "NULL_CHUNK_BYTES", 3 * bytes_per_sample + bytes_per_sample // 2)
        m.setattr(module, op, recorded)
        return null(), issued


def test_nulls_in_pieces_equal_the_single_call(monkeypatch):
    cuts = [(3, 0), (3, 3), (1, 6)]
    d, sizes = symmetric(65, 1, False), [2, 33, 64, 65]
    whole = K.null_sums(d, sizes, SAMPLES, SEED)
    got, issued = in_pieces(monkeypatch, K, "random_pair_sums", 8 * len(sizes), lambda: K.null_sums(d, sizes, SAMPLES, SEED))
    assert issued == cuts and whole.shape == (SAMPLES, len(sizes)) and np.array_equal(got, whole)
    assert np.array_equal(whole, K.random_pair_sums(d, sizes, SAMPLES, SEED).cpu().numpy())

    a, b = symmetric(65, 2, True), symmetric(65, 3, True)
    whole = MT.null_cross_sums(a, b, SAMPLES, SEED)
    got, issued = in_pieces(monkeypatch, MT, "cross_sums", 8, lambda: MT.null_cross_sums(a, b, SAMPLES, SEED))
    assert issued == cuts and whole.shape == (SAMPLES,) and np.array_equal(got, whole)
    assert np.array_equal(whole, MT.cross_sums(a, b, SAMPLES, SEED).cpu().numpy())

    rng = np.random.RandomState(4)
    order = E.profile_order(np.exp(rng.randn(2, 140)), [0, 1], np.sort(rng.permutation(140)[:130]))
    sizes = [1, 64, 65]
    whole = E.null_scores(order, sizes, SAMPLES, SEED)
    got, issued = in_pieces(monkeypatch, E, "random_enrichment_scores", 8 * len(sizes) * 2, lambda: E.null_scores(order, sizes, SAMPLES, SEED))
    assert issued == cuts and whole.shape == (2, SAMPLES, len(sizes)) and np.array_equal(got, whole)
    assert np.array_equal(whole, E.random_enrichment_scores(order, sizes, SAMPLES, SEED).cpu().numpy()) and not np.isnan(whole).any()
