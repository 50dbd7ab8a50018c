#!/usr/bin/env python3
"""Which genes does a treatment run through?  `python knockout.py -c config.json --triples pharmgkb_df.tsv` knocks every listed gene out of
the interactome and reports how far the drug's and the indication's diffusion profiles have moved apart;
`--drug DB... --indication C... --all-proteins` screens every protein for one pair.  The profiles of all knock-outs are columns of one
batched power iteration and the distances come from one launch per batch, in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.knockout import main

if __name__ == '__main__':
    main()
