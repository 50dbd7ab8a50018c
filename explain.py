#!/usr/bin/env python3
"""Which proteins and biological functions does a treatment run through?  `python explain.py -c config.json --drug DB... --indication C...`
lists the nodes the drug's and the indication's diffusion profiles rank highest, per node type, with their ranks in both and the ones they
share; `--pairs pairs.tsv` or `--treatments` counts the shared nodes of many pairs.  The top nodes of all referenced profiles come from one
exact selection launch and the overlaps from one more, in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.explain import main

if __name__ == '__main__':
    main()
