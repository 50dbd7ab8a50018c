#!/usr/bin/env python3
"""The third validation of the multiscale interactome, for which the reference ships the table and no code: `python drug_classes.py -c
config.json --classes data/drug_classification_df.tsv` asks of every ATC class whether its drugs' diffusion profiles are nearer to each
other than those of random drug sets of the same size (mean pairwise distance, z, empirical p, Benjamini-Hochberg q per level).  The
distances and the sums over the classes and the random sets are computed in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.classes import main

if __name__ == '__main__':
    main()
