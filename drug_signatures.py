#!/usr/bin/env python3
"""The multiscale interactome's validation against the Connectivity Map, for which the reference ships the table and no code: `python
drug_signatures.py -c config.json --signatures data/bcm_df.tsv` asks whether drugs with similar diffusion profiles have similar
gene-expression signatures: the correlation of the two drug x drug distance matrices over their pairs, tested by Mantel's permutation test
(r, z, empirical p).  The distances and the permuted cross-product sums of the null are computed in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.signatures import main

if __name__ == '__main__':
    main()
