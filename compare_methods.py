#!/usr/bin/env python3
"""What the reference's `median auc: X, mean auc: Y` leaves open: `python compare_methods.py --tables diffusion=a.tsv gcn=b.tsv` reads the
tables `evaluate_auc.py --per-indication` wrote, gives every method's median and mean a bootstrap percentile interval over the indications
and tests every method against the baseline on the per-indication differences (mean and median difference with intervals, two-sided
sign-flip p-values, wins / losses / ties).  The resamples and the sign flips are computed in a HIP kernel on the GPU."""
from gcn_drug_repurposing_amd.resample import main

if __name__ == '__main__':
    main()
