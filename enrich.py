#!/usr/bin/env python3
"""Which biological functions does a treatment act through as a whole?  `python enrich.py -c config.json --node DB... --node C...` scores
every function's protein set (or every indication's, every drug's, or the sets of a .gmt file) against the nodes' diffusion profiles:
the preranked gene-set enrichment score, its empirical p against random protein sets of the same size, the normalised score, the
Benjamini-Hochberg q and the leading edge.  The order of the profiles and the scores of the sets and of the random sets are computed in
HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.enrich import main

if __name__ == '__main__':
    main()
