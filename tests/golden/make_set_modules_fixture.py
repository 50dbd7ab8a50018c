"""Writes tests/golden/set_modules_2016.npz from tests/golden/proximity_2016.npz alone: the mirror's (tests/set_modules_mirror.py)
component tables of the 78 disease gene sets and their 1,000 degree-matched random sets (side 1, seed 452456, min_bin_size 100: the sets
proximity.py scores against), and the observed triples of the 238 drug target sets.  About a minute on one core.

  disease        int16 [3, 78, 1001]   lcc, n_comp, n_edges; sample 0 is the set itself
  disease_short  int16 [78]            random sets that came out a member short
  drug           int16 [3, 238]        lcc, n_comp, n_edges of the drug target sets themselves

Run from the repository root: python tests/golden/make_set_modules_fixture.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import proximity_mirror as PM  # noqa: E402
import set_modules_mirror as M  # noqa: E402


def main():
    fx = PM.Fixture()
    net = fx.net
    bin_list, node_bin, diseases, drugs = M.fixture_inputs(fx)
    tables, short = [], []
    for j, members in enumerate(diseases):
        t, sizes = M.module_nulls(net.rowptr, net.col, members, node_bin, bin_list, M.SEED, 1, j, M.N_RANDOM)
        tables.append(t)
        short.append(int((sizes[1:] < sizes[0]).sum()))
        print(f"disease {j}: n={len(members)} lcc={t[0, 0]} n_comp={t[1, 0]} n_edges={t[2, 0]}", flush=True)
    disease = np.stack(tables, axis=1)
    drug = np.stack(M.table(net.rowptr, net.col, drugs)[:3])
    assert disease.max() < 2 ** 15 and drug.max() < 2 ** 15
    out = os.path.join(HERE, "set_modules_2016.npz")
    np.savez(out, **PM.pack({"disease": disease.astype(np.int16), "disease_short": np.array(short, np.int16), "drug": drug.astype(np.int16)}))
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
