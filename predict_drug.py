#!/usr/bin/env python3
"""Drop-in for predict_drug.py: `python predict_drug.py -c config.json` ranks the drug candidates for a disease node and writes the
reference's table (drug name, proximity, connected proteins, shortest path to the query, path length).  The shortest paths run in HIP
kernels on the GPU; --query ranks for any node, --protein-table also writes run_covid.py's protein table."""
from gcn_drug_repurposing_amd.predict import main

if __name__ == '__main__':
    main()
