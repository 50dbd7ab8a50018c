#!/usr/bin/env python3
"""Drop-in for method/test_proximity.py (Guney et al. 2016 network proximity, toolbox wrappers.calculate_proximity): scores every
drug-disease pair of a table, or all of them, with d, z and pval per measure.  Distances, random sets and scoring run in HIP kernels."""
from gcn_drug_repurposing_amd.proximity_cli import main

if __name__ == '__main__':
    main()
