#!/usr/bin/env python3
"""The seed connector algorithm (Wang and Loscalzo 2018): `python seed_connectors.py --network network.sif --diseases disease_genes.tsv`
joins the fragments of every disease's genes on the interactome, one connector per step, each step the node that most enlarges the
largest connected component; --summary compares the seeds joined with degree-matched random sets, --connectors lists every step.
Every gene set and every random set grows in its own workgroup of one HIP kernel on the GPU."""
from gcn_drug_repurposing_amd.connectors_cli import main

if __name__ == '__main__':
    main()
