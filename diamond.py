#!/usr/bin/env python3
"""DIAMOnD (Ghiassian, Menche and Barabasi 2015): `python diamond.py --network network.sif --diseases disease_genes.tsv` grows a module
from every disease's genes on the interactome, one node per step, each step the node whose links into the module are the most
significant under the hypergeometric null; --summary adds the largest connected component before and after, --holdout a leave-out
validation.  Every seed set grows in its own workgroup of one HIP kernel launch on the GPU."""
from gcn_drug_repurposing_amd.diamond_cli import main

if __name__ == '__main__':
    main()
