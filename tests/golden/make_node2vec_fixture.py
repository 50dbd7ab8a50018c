"""Writes tests/golden/node2vec_msi_small.npz: the transition probabilities of the reference's node2vec walker on the weighted,
directed msi_small graph, reconstructed from the reference's own alias tables.

Imports multiscale/openne/walker.py from a reference checkout by file path (it needs numpy only; networkx builds the graph), runs
Walker(...).preprocess_transition_probs() at (p, q) = (0.25, 0.25) and (4, 0.5), and stores for every node cur the probability of
each successor (alias_nodes: step 1 of a walk) and for every edge (prev, cur) the probability of each successor of cur
(alias_edges: later steps).  An alias table (J, q) over K outcomes draws k with probability (min(q[k], 1) + sum over j with
J[j] = k of (1 - min(q[j], 1))) / K (alias_draw).  Nodes are numbered in MsiGraph.names order.

usage: python tests/golden/make_node2vec_fixture.py <reference root>
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
CASES = ((0.25, 0.25), (4.0, 0.5))


def alias_probs(J, q):
    K = len(J)
    qc = np.minimum(np.asarray(q, np.float64), 1.0)
    p = qc.copy()
    np.add.at(p, np.asarray(J), 1.0 - qc)
    return p / K


def main(ref_root):
    import networkx as nx

    from gcn_drug_repurposing_amd.msi import COVID_WEIGHTS, MsiGraph
    spec = importlib.util.spec_from_file_location("ref_walker", os.path.join(ref_root, "multiscale", "openne", "walker.py"))
    walker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(walker)
    d = os.path.join(HERE, "msi_small")
    files = {f[:-4]: os.path.join(d, f) for f in os.listdir(d) if f.endswith(".tsv")}
    g = MsiGraph().load(files).weight_graph(COVID_WEIGHTS)
    names = g.names
    idx = {n: i for i, n in enumerate(names)}
    G = nx.DiGraph()
    G.add_nodes_from(names)
    for u, succ in g.adj.items():
        for v, w in succ.items():
            G.add_edge(u, v, weight=w)

    class Graph:  # the attributes Walker reads from OpenNE's Graph
        pass
    gr = Graph()
    gr.G, gr.node_size, gr.look_up_dict = G, G.number_of_nodes(), idx
    out = {"names": np.array(names), "p": np.array([c[0] for c in CASES]), "q": np.array([c[1] for c in CASES])}
    for ci, (p, q) in enumerate(CASES):
        w = walker.Walker(gr, p=p, q=q, workers=1)
        w.preprocess_transition_probs()
        cur, nxt, prob = [], [], []
        for node in G.nodes():
            nb = list(G.neighbors(node))
            if nb:
                pr = alias_probs(*w.alias_nodes[node])
                cur += [idx[node]] * len(nb)
                nxt += [idx[x] for x in nb]
                prob += list(pr)
        out[f"node_cur_{ci}"], out[f"node_next_{ci}"], out[f"node_prob_{ci}"] = np.array(cur), np.array(nxt), np.array(prob)
        prev, cur, nxt, prob = [], [], [], []
        for (a, b), tab in w.alias_edges.items():
            nb = list(G.neighbors(b))
            if nb:
                pr = alias_probs(*tab)
                prev += [idx[a]] * len(nb)
                cur += [idx[b]] * len(nb)
                nxt += [idx[x] for x in nb]
                prob += list(pr)
        out[f"edge_prev_{ci}"], out[f"edge_cur_{ci}"] = np.array(prev, np.int32), np.array(cur, np.int32)
        out[f"edge_next_{ci}"], out[f"edge_prob_{ci}"] = np.array(nxt, np.int32), np.array(prob)
    np.savez_compressed(os.path.join(HERE, "node2vec_msi_small.npz"), **out)
    print("wrote node2vec_msi_small.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
