"""CPU: the host side of knockout.py that needs no GPU -- the chunk plan (baselines with their knock-outs, columns computed once, the
two knocked-out columns side by side, from an even column in a screen), the triples table and its skip counts, the TSV writer, and the refusals of
the command line that come before the GPU is touched."""
import io
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluate_fixture as EF  # noqa: E402
import knockout_mirror as KM  # noqa: E402

from gcn_drug_repurposing_amd import knockout as K  # noqa: E402


def test_chunk_plan():
    triples = [("D1", "I1", "g%d" % t) for t in range(7)] + [("D1", "I2", "g0"), ("D2", "I1", "g3"), ("D1", "I1", "g2")]
    for cap in (4, 5, 6, 9, 4096):
        chunks = K.plan_chunks(triples, cap)
        assert [r[:3] for _, _, rows in chunks for r in rows] == triples                 # every triple once, in order
        for cols, pairs, rows in chunks:
            assert len(cols) <= cap
            named = [c for c in cols if c[1] is not None]
            assert len(set(named)) == len(named)                                         # a (start, gene) column is computed once
            for d, i, g, before, after, sd, si, kd, ki in rows:
                assert cols[pairs[before][0]] == (d, None) and cols[pairs[before][1]] == (i, None)   # the baselines are in the chunk
                assert (cols[kd], cols[ki]) == ((d, g), (i, g)) and pairs[after] == (kd, ki)
                assert pairs[sd] == (pairs[before][0], kd) and pairs[si] == (pairs[before][1], ki)
            assert len(set(pairs)) == len(pairs)
    cols, pairs, rows = K.plan_chunks(triples[:7], 4096)[0]
    assert all(kd % 2 == 0 and ki == kd + 1 for *_, kd, ki in rows)                      # one 16-byte load per knocked-out pair
    with pytest.raises(K.KnockoutError, match="max_columns=3"):
        K.plan_chunks(triples, 3)


def test_triples_table_and_skip_counts(tmp_path):
    g = KM.small_graph()
    path = tmp_path / "t.tsv"
    path.write_text("drug\tdrug_name\tindication\tindication_name\tgene\tgene_name\n"
                    "DB00003\tx\tC0000000\ty\t151\tz\n"
                    "DB00003\tx\tC0000000\ty\t151\tz\n"            # a repeated triple is answered once
                    "DB99999\tx\tC0000000\ty\t151\tz\n"
                    "DB00003\tx\tC9999999\ty\t151\tz\n"
                    "DB00003\tx\tC0000004\ty\t999999\tz\n"
                    "DB00003\tx\tC0000004\ty\tC0000000\tz\n"       # not a protein
                    "C0000000\tx\tDB00003\ty\t151\tz\n"            # the columns swapped
                    "DB00003\tx\tNodeCovid\ty\t104\tz\n")
    triples = K.read_triples(str(path))
    assert len(triples) == 8 and triples[0] == ("DB00003", "C0000000", "151")
    err = io.StringIO()
    assert K.usable_triples(g, triples, err) == [("DB00003", "C0000000", "151"), ("DB00003", "NodeCovid", "104")]
    assert err.getvalue().splitlines() == ["knockout: skipped 2 triples: drug not in the graph",
                                           "knockout: skipped 2 triples: gene not in the graph",
                                           "knockout: skipped 1 triples: indication not in the graph"]
    bad = tmp_path / "bad.tsv"
    bad.write_text("drug\tgene\n")
    with pytest.raises(K.KnockoutError, match="needs the columns drug, indication and gene"):
        K.read_triples(str(bad))


def test_tsv_writer(tmp_path):
    rec = [{"drug": "DB1", "indication": "C1", "gene": "7", "gene name": None, "dist_before": 0.1, "dist_after": 0.30000000000000004,
            "delta": 0.20000000000000004, "shift_drug": 0.0, "shift_indication": float("nan"), "iterations_drug": 12,
            "iterations_indication": 13}]
    K.write_records(str(tmp_path / "k.tsv"), rec)
    lines = (tmp_path / "k.tsv").read_text().split("\n")
    assert lines[0].split("\t") == K.HEADER and lines[2] == ""
    assert lines[1].split("\t") == ["DB1", "C1", "7", "NA", "0.1", "0.30000000000000004", "0.20000000000000004", "0.0", "nan", "12", "13"]


def test_command_line_refusals_before_the_gpu(tmp_path):
    cfg = EF.stage(tmp_path, "diffusion", with_embs=False)
    cases = [(dict(), "give either --triples"),
             (dict(triples="t.tsv", drug="DB00003"), "give either --triples"),
             (dict(drug="DB00003", indication="C0000000"), "screen mode needs"),
             (dict(drug="DB00003", genes="g.txt"), "screen mode needs"),
             (dict(drug="DB00003", indication="C0000000", genes="g.txt", all_proteins=True), "screen mode needs"),
             (dict(triples="t.tsv", top=3), "--top K needs the screen mode"),
             (dict(drug="DB00003", indication="C0000000", all_proteins=True, top=0), "--top K needs"),
             (dict(triples="t.tsv", metric="chebyshev"), "'chebyshev' is unknown")]
    for kw, message in cases:
        with pytest.raises(K.KnockoutError, match=message):
            K.run(cfg, **kw)
    with pytest.raises(SystemExit) as e:
        K.main(["-c", cfg, "--triples", "t.tsv", "--metric", "chebyshev"])
    assert e.value.code == 2
