#!/usr/bin/env python3
"""The comparison the multiscale interactome rests on and the reference never makes: `python compare_profiles.py -c config.json --metric
correlation --rows indications --cols drugs` lists, for every indication, the drugs whose diffusion profiles are nearest to its own
(`--rows drugs --cols drugs`: the drug-drug similarity).  The distances are computed in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.compare import main

if __name__ == '__main__':
    main()
