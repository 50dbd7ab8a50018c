#!/usr/bin/env python3
"""The command the reference's interpret.py describes and never wrote: `python interpret.py -c config.json` traces the ranked drug
candidates to the query node -- how many shortest paths connect each drug to it, the nodes and edges on them with the share of the
paths through each, the path the model's proximities favour, and the mediators of the query over the traced drugs.  The counts and the
between pass run in HIP kernels on the GPU."""
from gcn_drug_repurposing_amd.interpret import main

if __name__ == '__main__':
    main()
