#!/usr/bin/env python3
"""Cuts the head of the reference's Connectivity Map signature table (data/bcm_df.tsv: 63 drugs, one row each, the columns drug, drug_name,
sig_id, cell, dose, time and one column per landmark gene, 978 Entrez ids) into a data-only fixture, tests/golden/bcm_signatures_head.tsv:
the header and the first ROWS rows, verbatim, cut to the six leading columns and the first GENES gene columns.

    python tests/golden/make_signature_fixture.py <reference root>      (tests/test_mantel.py reads it with signatures.read_signatures)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, GENES, LEAD = 5, 16, 6


def main():
    path = os.path.join(sys.argv[1], "data", "bcm_df.tsv")
    with open(path, encoding="utf-8", newline="") as f:
        lines = [f.readline() for _ in range(ROWS + 1)]
    with open(os.path.join(HERE, "bcm_signatures_head.tsv"), "w", encoding="utf-8", newline="") as f:
        for line in lines:
            f.write("\t".join(line.rstrip("\r\n").split("\t")[:LEAD + GENES]) + "\n")


if __name__ == "__main__":
    main()
