#!/usr/bin/env python3
"""Random walk with restart (network propagation): `python rwr.py --network network.sif --diseases disease_genes.tsv` ranks the genes of
the interactome by how often a walk that restarts on a disease's genes visits them; --n-random adds the z-score against degree-matched
random sets, --holdout the leave-out validation whose recovery.tsv sits beside diamond.py's.  Every seed set walks in its own workgroup
of one HIP kernel launch on the GPU."""
from gcn_drug_repurposing_amd.rwr_cli import main

if __name__ == '__main__':
    main()
