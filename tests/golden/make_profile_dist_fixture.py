"""Writes tests/golden/profile_dist_msi_small.npz: what scipy and sklearn say about distances between the reference's own diffusion profiles.

It needs no run of the reference: tests/golden/diffusion_msi_small.npz already holds the reference's profiles of all 21 start nodes of the
msi_small tables (12 drugs, 8 indications, NodeCovid; 111 nodes).  Per metric of diffusion.METRICS this writes
  d_<metric>    scipy.spatial.distance.cdist of the 21 profiles with themselves, rows / columns in `names` order (= the fixture's `starts`)
  deg_<metric>  cdist of the degenerate 4 x 4 case `deg_x` (Canberra's 0 / 0 terms, the NaN pattern of cosine and correlation)
  auc_<metric>  sklearn.metrics.roc_auc_score per indication of `auc_indications`, every drug scored by minus its distance to the indication,
                labels from evaluate_msi_small/drug_indication_df.tsv; indications and drugs in the graph's node order, as evaluate_auc.py
                walks them
and asserts that in every indication's row and every metric the smallest gap between two different drugs' distances is at least 1e-7 of the
row's largest distance, the condition under which a ranking (and so an AUC) cannot depend on the summation order or on profiles that
differ from the reference's by 1e-13.

    python tests/golden/make_profile_dist_fixture.py
"""
import os
import sys

import numpy as np
from scipy.spatial.distance import cdist
from sklearn.metrics import roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

METRICS = ("cityblock", "euclidean", "canberra", "cosine", "correlation")
DEGENERATE = np.array([[0, 0, 1, 2], [0, 0, 0, 0], [1, 1, 1, 1], [.5, 0, 1, 2]], dtype=np.float64)
MIN_GAP = 1e-7


def main():
    from gcn_drug_repurposing_amd.consumer import read_drug_indication_tsv
    from gcn_drug_repurposing_amd.msi import COMPONENTS, DRUG, INDICATION, MsiGraph
    z = np.load(os.path.join(HERE, "diffusion_msi_small.npz"))
    names = [str(s) for s in z["starts"]]
    prof = np.asarray(z["profiles"], dtype=np.float64)
    ev = np.load(os.path.join(HERE, "evaluate_msi_small", "diffusion_profiles.npz"))
    assert [str(n) for n in ev["nodelist"]] == [str(n) for n in z["nodelist"]]
    for i, p in zip(ev["indications"], ev["profiles"]):          # the evaluate fixture is the same graph: its profiles are these rows
        assert np.array_equal(p, prof[names.index(str(i))])
    assert prof.min() > 0                                          # no profile entry is zero
    g = MsiGraph().load({n: os.path.join(HERE, "msi_small", n + ".tsv") for n, _, _ in COMPONENTS})
    nodelist = [str(n) for n in z["nodelist"]]
    drugs = [n for n in nodelist if g.type.get(n) == DRUG]
    inds = [n for n in nodelist if g.type.get(n) == INDICATION]
    assert sorted(drugs + inds) == sorted(names)
    positives = read_drug_indication_tsv(os.path.join(HERE, "evaluate_msi_small", "drug_indication_df.tsv"))
    di = [names.index(d) for d in drugs]
    out = {"names": np.asarray(names), "drugs": np.asarray(drugs), "deg_x": DEGENERATE}
    kept = [i for i in inds if 0 < sum(d in positives.get(i, ()) for d in drugs) < len(drugs)]
    out["auc_indications"] = np.asarray(kept)
    for m in METRICS:
        d = cdist(prof, prof, m)
        out["d_" + m] = d
        with np.errstate(invalid="ignore", divide="ignore"):
            out["deg_" + m] = cdist(DEGENERATE, DEGENERATE, m)
        aucs, gaps = [], []
        for i in inds:
            row = d[names.index(i), di]
            gaps.append(np.diff(np.sort(row)).min() / row.max())
            if i in kept:
                aucs.append(roc_auc_score([d_ in positives[i] for d_ in drugs], -row))
        assert min(gaps) >= MIN_GAP, (m, min(gaps))
        out["auc_" + m] = np.asarray(aucs)
        print(f"{m:12s} median / mean AUC {np.median(aucs):.4f} / {np.mean(aucs):.4f}   smallest relative gap {min(gaps):.2e}")
    np.savez_compressed(os.path.join(HERE, "profile_dist_msi_small.npz"), **out)


if __name__ == "__main__":
    main()
