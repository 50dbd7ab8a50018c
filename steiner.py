#!/usr/bin/env python3
"""Approximate Steiner trees (Kou, Markowsky and Berman 1981; Mehlhorn 1988): `python steiner.py --network network.sif --diseases
disease_genes.tsv` connects every disease's genes on the interactome by the smallest subnetwork the 2(1 - 1/l) approximation finds;
--nodes names the connector (Steiner) nodes, --summary compares their number and the tree's length with degree-matched random sets.
Every gene set and every random set is connected in its own workgroup of one HIP kernel on the GPU."""
from gcn_drug_repurposing_amd.steiner_cli import main

if __name__ == '__main__':
    main()
