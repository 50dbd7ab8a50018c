#!/usr/bin/env python3
"""Packs the reference's drug-class table (data/drug_classification_df.tsv: 3,987 rows of DrugBank id, ATC code and the four ATC levels with
their names) into a data-only fixture, tests/golden/atc_classes.npz: the drug ids in order of first appearance, and per level the class
codes, their names and each class's drugs as indices into that list (CSR), as classes.read_classes reads them from the table.

    python tests/golden/make_atc_fixture.py <reference root>      (tests/class_cohesion_mirror.atc_fixture() is the reader)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gcn_drug_repurposing_amd.classes import read_classes  # noqa: E402


def text(items):
    return np.frombuffer("\n".join(items).encode(), dtype=np.uint8)


def main():
    path = os.path.join(sys.argv[1], "data", "drug_classification_df.tsv")
    drugs, table = read_classes(path, [1, 2, 3, 4])
    at = {n: i for i, n in enumerate(drugs)}
    out = {"rows": np.int64(sum(1 for _ in open(path)) - 1), "drugs": text(drugs)}
    for k, by_code in table.items():
        codes = list(by_code)
        out[f"codes_{k}"], out[f"names_{k}"] = text(codes), text([by_code[c][0] for c in codes])
        out[f"ptr_{k}"] = np.cumsum([0] + [len(by_code[c][1]) for c in codes]).astype(np.int32)
        out[f"members_{k}"] = np.asarray([at[n] for c in codes for n in by_code[c][1]], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "atc_classes.npz"), **out)


if __name__ == "__main__":
    main()
