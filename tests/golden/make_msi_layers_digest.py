#!/usr/bin/env python3
"""Golden digest of the reference's MSI tables, for tests/test_msi.py::test_real_layer_fixture_is_the_reference_tables_verbatim:
per edge table the row count and the sha256 of its (node_1, node_2) columns in file row order, one "node_1\\tnode_2\\n" line per
row; for data/drug_indication_df.tsv the count and sha256 of its distinct (indication, drug) pairs, sorted, one
"indication\\tdrug\\n" line per pair.  Hashes only, no table content.

    python tests/golden/make_msi_layers_digest.py <reference checkout>
"""
import csv
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "msi_real_layers_digest.json")
TABLES = ("drug_to_protein", "indication_to_protein", "covid_to_protein", "protein_to_functional_pathway",
          "functional_pathway_to_functional_pathway")


def digest(lines):
    h = hashlib.sha256()
    for line in lines:
        h.update(line.encode())
    return h.hexdigest()


def main():
    data = os.path.join(sys.argv[1], "data")
    out = {}
    for stem in TABLES:
        with open(os.path.join(data, stem + ".tsv"), newline="") as f:
            rows = list(csv.reader(f, delimiter="\t"))[1:]
        out[stem] = {"rows": len(rows), "sha256": digest(f"{r[0]}\t{r[1]}\n" for r in rows)}
    with open(os.path.join(data, "drug_indication_df.tsv"), newline="") as f:
        pairs = sorted({(r[2], r[0]) for r in list(csv.reader(f, delimiter="\t"))[1:]})
    out["drug_indication_df"] = {"rows": len(pairs), "sha256": digest(f"{a}\t{b}\n" for a, b in pairs)}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
