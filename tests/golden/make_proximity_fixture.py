"""Writes tests/golden/proximity_2016.npz from the reference's 2016 data (Guney et al. 2016; the reference's method/test_proximity.py):

  python tests/golden/make_proximity_fixture.py <reference root>

Data only, every column lzma-packed (proximity_mirror.pack / unpack; about 0.65 MB in all):
  * net_genes / net_cnt / net_dv: network/network.sif (the relation column dropped) as its genes in order of first appearance and
    the unique undirected edges u <= v by that order, per-node counts and delta-coded columns (proximity_mirror.encode_network);
  * the table's 238 drugs and 78 diseases: names and gene-id lists in CSR form (drug_*, disease_*), the gene ids as in the source
    files (before the LCC intersection);
  * pair_drug / pair_disease [18564]: the tables' row order (identical in all five) as indices into those lists; flag: the table's
    flag column is True (known indication); n_target / n_disease;
  * <measure>_d (fp64, as parsed from the text) and <measure>_z_e4 = round(z * 1e4) for closest, shortest, kernel, center,
    separation.  pval is not stored: it is Phi(z) in every table (to 1.6e-12);
  * spread_<measure> [3]: percentiles 50/90/99 of |z(seed A) - z(seed B)| of tests/proximity_mirror.py at n_random = 1000 over
    SPREAD_PAIRS sampled pairs (the Monte Carlo noise the device's z is judged against).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

MEASURES = ("closest", "shortest", "kernel", "center", "separation")
SPREAD_PAIRS = 200
SEEDS = (452456, 1)


def read_table(path):
    with open(path) as f:
        head = f.readline().split()
        rows = [line.split() for line in f if line.strip()]
    col = {h: i for i, h in enumerate(head)}
    return rows, col


def main(ref):
    from gcn_drug_repurposing_amd import proximity as P
    import proximity_mirror as M
    data = os.path.join(ref, "2016data")
    edges = []
    with open(os.path.join(data, "network", "network.sif")) as f:
        for line in f:
            p = line.split()
            if p:
                edges.append((int(p[0]), int(p[2])))
    edges = np.array(edges, np.int64)
    drugs = P.load_drug_targets(os.path.join(data, "target", "drug_to_geneids.pcl.all"))
    diseases = P.load_disease_genes(os.path.join(data, "disease", "disease_genes.tsv"))
    genes, cnt, dv = M.encode_network(edges)
    out = {"net_genes": genes, "net_cnt": cnt, "net_dv": dv}
    tables = {m: read_table(os.path.join(data, "proximity", f"{m}.dat")) for m in MEASURES}
    rows, col = tables["closest"]
    drug_names = sorted({r[col["group"]] for r in rows})
    dis_names = sorted({r[col["disease"]] for r in rows})
    for tag, names, src in (("drug", drug_names, drugs), ("disease", dis_names, diseases)):
        lists = [sorted(int(g) for g in src[nm]) for nm in names]
        out[f"{tag}_names"] = np.array(names)
        out[f"{tag}_ptr"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        out[f"{tag}_genes"] = np.concatenate(lists).astype(np.int32)
    di, si = {n: i for i, n in enumerate(drug_names)}, {n: i for i, n in enumerate(dis_names)}
    out["pair_drug"] = np.array([di[r[col["group"]]] for r in rows], np.uint8)
    out["pair_disease"] = np.array([si[r[col["disease"]]] for r in rows], np.uint8)
    out["flag"] = np.array([r[col["flag"]] == "True" for r in rows])
    out["n_target"] = np.array([int(r[col["n.target"]]) for r in rows], np.int16)
    out["n_disease"] = np.array([int(r[col["n.disease"]]) for r in rows], np.int16)
    for m in MEASURES:
        rows_m, col_m = tables[m]
        assert [(r[col_m["group"]], r[col_m["disease"]]) for r in rows_m] == [(r[col["group"]], r[col["disease"]]) for r in rows]
        d, z = (np.array([float(r[col_m[f]]) for r in rows_m]) for f in ("d", "z"))
        assert np.all(np.abs(z) < 2 ** 31 / M.Z_SCALE)
        out[f"{m}_d"] = d
        out[f"{m}_z_e4"] = np.round(z * M.Z_SCALE).astype(np.int32)

    # the Monte Carlo spread of z between two seeds of the mirror, all five measures on the same sampled pairs
    u, v = M.decode_network(genes, cnt, dv)
    net = P.Network(np.stack([u, v], 1).ravel(), np.stack([v, u], 1).ravel(), [str(g) for g in genes])
    print(f"LCC {net.n} nodes; all-pairs BFS on the host ...", flush=True)
    D = np.concatenate([M.bfs_rows(net.rowptr, net.col, np.arange(c, min(c + 512, net.n))) for c in range(0, net.n, 512)])
    dist = lambda T, S: D[np.ix_(np.asarray(T), np.asarray(S))]  # noqa: E731
    bl = M.bins(net.degree, 100)
    nb = M.bin_of(bl, net.n)
    rng = np.random.RandomState(0)
    pick = rng.choice(len(rows), SPREAD_PAIRS, replace=False)
    zs = {m: np.zeros((2, SPREAD_PAIRS)) for m in MEASURES}
    for q, p in enumerate(pick):
        i, j = int(out["pair_drug"][p]), int(out["pair_disease"][p])
        T = net.node_set(str(g) for g in out["drug_genes"][out["drug_ptr"][i]:out["drug_ptr"][i + 1]])
        S = net.node_set(str(g) for g in out["disease_genes"][out["disease_ptr"][j]:out["disease_ptr"][j + 1]])
        for a, seed in enumerate(SEEDS):
            res = M.proximity(dist, T, S, nb, bl, seed, i, j, 1000)
            for m in MEASURES:
                zs[m][a, q] = res[m][3]
        if q % 20 == 0:
            print(f"spread pair {q}/{SPREAD_PAIRS}", flush=True)
    for m in MEASURES:
        out[f"spread_{m}"] = np.percentile(np.abs(zs[m][0] - zs[m][1]), [50, 90, 99])
        print(m, out[f"spread_{m}"])
    out["spread_pairs"] = pick.astype(np.int32)
    path = os.path.join(HERE, "proximity_2016.npz")
    np.savez(path, **M.pack(out))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
