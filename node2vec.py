#!/usr/bin/env python3
"""Drop-in for `python -m openne --method node2vec ...` (multiscale/openne/__main__.py): reads an edgelist, writes the .embs.txt the
trainer reads (train.py --emb-file).  Walks and skip-gram run in HIP kernels on the GPU; no gensim / OpenNE / TensorFlow."""
from gcn_drug_repurposing_amd.node2vec_cli import main

if __name__ == '__main__':
    main()
