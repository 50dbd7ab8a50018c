"""enrich.py: does a biological function, an indication's protein set or a drug's targets as a whole sit higher in a diffusion profile than
random protein sets of the same size, and how sure is that?  explain.py lists the top nodes of a profile; this scores *sets* against it:
preranked gene-set enrichment, the Kolmogorov-Smirnov-like running sum of Subramanian et al. 2005 with a gene-set permutation null.  The
reference ships the sets (data/protein_to_functional_pathway.tsv) and no code that scores one.

The order of a profile over the universe (the protein nodes), the scores of the listed sets and the scores of the random sets are HIP
kernels (csrc/enrich.hip; no CPU fallback): gss_profile_order, gss_enrich_lists, gss_enrich_random -- one seeded permutation of the
universe per sample, whose first m places are the random set of size m, so one launch serves every set size and every profile.  What comes
back is [profiles][samples][sizes] scores; the empirical p, the normalised score, the Benjamini-Hochberg q and the leading edge are host numpy."""
from __future__ import annotations

import argparse
import collections
import json
import sys

import numpy as np

from . import _lib, predict
from ._nulls import NULL_CHUNK_BYTES, benjamini_hochberg, chunked_null, device_lists, int32_array  # noqa: F401
from .msi import DRUG, FUNCTIONAL_PATHWAY, INDICATION, PROTEIN
from .predict import PredictError, write_tsv

MAX_SET = 1024                # gss_enrich_lists sorts a set's members in LDS
MAX_UNIVERSE = 65536          # gss_profile_order counts in chunks, quadratic in M / chunk
BUILT_IN_SETS = {"functions": FUNCTIONAL_PATHWAY, "indications": INDICATION, "drugs": DRUG}
HEADER = ["node", "node_name", "set", "set_name", "size", "es", "nes", "p", "q", "lead_size", "lead"]

# pos: device int32 [profiles][M], w: device fp64 [profiles][M] (gss_profile_order's outputs); universe: host int32 [M]
Order = collections.namedtuple("Order", ["pos", "w", "universe"])


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------

def _check_order(order, who):
    import torch
    if (not isinstance(order, Order) or not isinstance(order.pos, torch.Tensor) or not isinstance(order.w, torch.Tensor) or order.pos.dim() != 2
            or order.pos.dtype != torch.int32 or order.w.dtype != torch.float64 or order.pos.shape != order.w.shape or not order.pos.is_cuda
            or not order.w.is_cuda or not order.pos.is_contiguous() or not order.w.is_contiguous()):
        raise ValueError(f"{who}: order must be what profile_order returned (device tensors pos int32 and w fp64, both [profiles][M])")
    return order.pos.shape


def profile_order(profiles, cols, universe, device="cuda"):
    """the order of diffusion profiles over a universe of nodes -> Order(pos, w, universe): for profile cols[j] and place u (an index into
    universe), pos[j][u] = the place of u in np.argsort(-profile[universe], kind="stable") -- descending value, ties by the smaller
    place, exactly -- and w[j][u] = |profile[universe[u]]| (gss_profile_order).  `profiles` is what diffusion.top_nodes accepts: the
    device tensor x [N][kpad] (used in place; cols are column indices), a host array [K][N] (cols index its rows) or a {name: vector} dict
    (cols are names); cols may repeat and come in any order, None means every profile (not for a dict).  universe: strictly ascending
    node indices in [0, N), 2 .. 65,536 of them.  A profile with a NaN at a universe node has pos = -1 and w = NaN everywhere.  No CPU
    fallback."""
    import torch

    from .diffusion import _device_list, _profile_source, _workspace
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("the order of a profile is computed on the GPU only (no CPU fallback)")
    n, (c,), upload = _profile_source(profiles, (cols,), ("column",), "profile_order")
    if n < 1:
        raise ValueError("profile_order: the profiles are empty")
    uni = int32_array("universe", universe, "profile_order")
    M, nc = len(uni), len(c)
    x = upload(dev)
    pos = torch.empty(nc, M, dtype=torch.int32, device=x.device)
    w = torch.empty(nc, M, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.gss_profile_order_workspace_bytes(M, nc))
        ws, lst = _workspace(max(need, 256), x.device), _device_list(c, x.device)
        d_uni = torch.from_numpy(uni if M else np.zeros(1, dtype=np.int32)).to(x.device)
        _lib.check(lib.gss_profile_order(n, x.data_ptr(), _lib.row_stride(x), nc, _lib.ptr(lst), M, d_uni.data_ptr(), pos.data_ptr(), w.data_ptr(),
                                         ws.data_ptr(), max(need, 256), _lib.current_stream()), "gss_profile_order")
    return Order(pos, w, uni)


def enrichment_scores(order, sets, weighted=True):
    """the enrichment score of each set in each profile -> device tensors (es fp64 [profiles][len(sets)], peak int32 [profiles][len(sets)]):
    the extreme of the running sum over the profile's order that steps up by w / (the set's total w) at a member (1 / size when
    weighted=False) and down by 1 / (M - size) elsewhere, and the member (counted in the profile's order, from 0) at which it is reached
    (gss_enrich_lists; the header states the arithmetic operation by operation, and a set has the same bits alone and among others).
    sets: sequences of distinct places in [0, M), 1 .. min(1024, M - 1) each.  A set whose members all weigh 0.0, and every set of a
    profile that holds a NaN, gives NaN and -1.  No CPU fallback."""
    import torch
    nc, M = _check_order(order, "enrichment_scores")
    hl = [int32_array(f"set {c}", l, "enrichment_scores") for c, l in enumerate(sets)]
    dev = order.pos.device
    es = torch.empty(nc, len(hl), dtype=torch.float64, device=dev)
    peak = torch.empty(nc, len(hl), dtype=torch.int32, device=dev)
    if not hl or nc == 0:
        return es, peak
    with torch.cuda.device(dev):
        d_ptr, d_idx = device_lists(hl, "enrichment_scores", "sets", dev)
        _lib.check(_lib.load().gss_enrich_lists(M, nc, order.pos.data_ptr(), order.w.data_ptr(), int(bool(weighted)), len(hl), d_ptr.data_ptr(),
                                                d_idx.data_ptr(), es.data_ptr(), peak.data_ptr(), _lib.current_stream()), "gss_enrich_lists")
    return es, peak


def random_enrichment_scores(order, sizes, samples, seed=0, first=0, perms=False, weighted=True):
    """the same scores over random sets -> device tensor fp64 [profiles][samples][len(sizes)]: entry (j, s - first, k) is the score in
    profile j of the first sizes[k] places of permutation number s of the M places, s = first .. first + samples - 1
    (gss_enrich_random: places sorted by the counter-based key of (seed, s, place), a pure function of its arguments -- a call equals the
    same samples in any split through `first`, and a size or a profile has the same bits alone and among others).  sizes: strictly
    ascending in [1, min(1024, M - 1)].  perms=True also returns the permutations' prefixes, device int32 [samples][sizes[-1]].  No CPU
    fallback."""
    import torch
    nc, M = _check_order(order, "random_enrichment_scores")
    hs = int32_array("sizes", sizes, "random_enrichment_scores")
    P, ns = int(samples), len(hs)
    dev = order.pos.device
    with torch.cuda.device(dev):
        es = torch.empty(nc, max(P, 0), ns, dtype=torch.float64, device=dev)
        d_sizes = torch.from_numpy(hs if ns else np.zeros(1, dtype=np.int32)).to(dev)
        perm = torch.empty(max(P, 0), int(hs[-1]) if ns and hs[-1] > 0 else 0, dtype=torch.int32, device=dev) if perms else None
        _lib.check(_lib.load().gss_enrich_random(M, nc, order.pos.data_ptr(), order.w.data_ptr(), int(bool(weighted)), _lib.seed64(seed),
                                                 int(first), P, ns, d_sizes.data_ptr(), es.data_ptr(), _lib.ptr(perm), _lib.current_stream()),
                   "gss_enrich_random")
    return (es, perm) if perms else es


def null_scores(order, sizes, samples, seed=0, weighted=True):
    """random_enrichment_scores brought to the host -> fp64 [profiles][samples][len(sizes)], in calls of at most NULL_CHUNK_BYTES of scores"""
    return chunked_null(lambda count, first: random_enrichment_scores(order, sizes, count, seed, first, weighted=weighted), samples,
                        8 * len(sizes) * max(1, order.pos.shape[0]), axis=1)


# ---- the statistics (host) -----------------------------------------------------------------------------------------------------------

def enrichment_stats(es, peak, sets, pos, sizes, null):
    """one profile: es [C] and peak [C] of the sets (lists of places), the profile's pos [M], against the null scores [P][len(sizes)] -> a
    list of dicts.  Per set, with t = column sizes.index(len(set)) of the null and "same sign" = t >= 0 for ES >= 0, t < 0 otherwise (a NaN
    never counts): n_same, p = (1 + #{same-sign t with |t| >= |ES|}) / (1 + n_same), nes = ES / np.mean(|same-sign t|) (nan when
    n_same = 0), q = benjamini_hochberg over the profile's sets with a finite ES, and lead = the leading edge: the members in the
    profile's order up to and including the peak for ES >= 0, from the peak on otherwise.  A set whose ES is NaN has n_same = 0, p = nes
    = q = nan and no leading edge."""
    col = {int(m): k for k, m in enumerate(sizes)}
    null, pos = np.asarray(null, dtype=np.float64), np.asarray(pos)
    out = []
    for e, pk, members in zip(es, peak, sets):
        e, pk = float(e), int(pk)
        if e != e:
            out.append({"n_same": 0, "p": float("nan"), "nes": float("nan"), "q": float("nan"), "lead": []})
            continue
        t = null[:, col[len(members)]]
        mag = np.abs(t[t >= 0] if e >= 0 else t[t < 0])
        n_same = len(mag)
        members = np.asarray(members, dtype=np.int64)
        by_pos = members[np.argsort(pos[members], kind="stable")]
        out.append({"n_same": n_same, "p": (1 + int(np.count_nonzero(mag >= abs(e)))) / (1 + n_same),
                    "nes": e / float(np.mean(mag)) if n_same else float("nan"), "q": float("nan"),
                    "lead": [int(u) for u in (by_pos[:pk + 1] if e >= 0 else by_pos[pk:])]})
    scored = [k for k, r in enumerate(out) if r["p"] == r["p"]]
    for k, q in zip(scored, benjamini_hochberg([out[k]["p"] for k in scored])):
        out[k]["q"] = float(q)
    return out


def enrichment(profiles, cols, universe, sets, samples, seed=0, weighted=True, return_null=False, device="cuda"):
    """sets: {name: places} or a sequence of place lists (places = indices into universe, each once, 1 .. min(1024, M - 1)) -> one dict
    per (profile, set), profiles outermost, both in the given order: "profile" (cols[j]), "set" (the name or the position), size, es,
    peak, n_same, p, nes, q, lead (enrichment_stats; lead as places) from profile_order, enrichment_scores of the sets and `samples`
    random sets per distinct set size (random_enrichment_scores with `seed`).  return_null=True: -> (records, sizes, null scores
    [profiles][samples][sizes] on the host)."""
    names = list(sets.keys()) if isinstance(sets, dict) else list(range(len(sets)))
    lists = [list(sets[k]) for k in names]
    M = len(np.asarray(universe).reshape(-1))
    for k, l in zip(names, lists):
        if not 1 <= len(l) <= min(MAX_SET, M - 1) or len(set(l)) != len(l):
            raise ValueError(f"enrichment: set {k!r} must list 1 .. min({MAX_SET}, M - 1 = {M - 1}) places, each once")
    if not lists:
        raise ValueError("enrichment: no set")
    if int(samples) < 1:
        raise ValueError(f"enrichment: samples={samples} must be at least 1")
    order = profile_order(profiles, cols, universe, device)
    sizes = sorted({len(l) for l in lists})
    es, peak = (t.cpu().numpy() for t in enrichment_scores(order, lists, weighted))
    null = null_scores(order, sizes, int(samples), seed, weighted)
    pos = order.pos.cpu().numpy()
    listed = list(cols) if cols is not None else list(range(pos.shape[0]))
    rec = []
    for j, col in enumerate(listed):
        for k, l, e, pk, r in zip(names, lists, es[j], peak[j], enrichment_stats(es[j], peak[j], lists, pos[j], sizes, null[j])):
            rec.append({"profile": col, "set": k, "size": len(l), "es": float(e), "peak": int(pk), **r})
    return (rec, sizes, null) if return_null else rec


# ---- the program ---------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: gene-set enrichment of diffusion profiles -- which functions, indications' "
                                            "or drugs' protein sets a profile ranks higher than random sets of their size (enrich.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--node", action="append", default=None, type=str, help="a drug or an indication whose diffusion profile is scored; repeat for more")
    p.add_argument("--sets", default="functions", type=str, help="functions: the proteins of each biological function; indications / drugs: the "
                   "proteins of each indication / drug; or a .gmt file (name, description, protein ids, tab-separated) (default: functions)")
    p.add_argument("--min-size", default=5, type=int, help="drop sets with fewer proteins in the universe (default: 5)")
    p.add_argument("--max-size", default=500, type=int, help=f"drop sets with more proteins, at most {MAX_SET} (default: 500)")
    p.add_argument("--unweighted", action="store_true", help="every member steps the running sum by 1 / size (default: by its share of the profile)")
    p.add_argument("--samples", default=1000, type=int, help="random protein sets per set size (default: 1000)")
    p.add_argument("--seed", default=0, type=int, help="seed of the random sets (default: 0)")
    p.add_argument("--top", default=None, type=int, help="keep the first K rows of each node (default: all)")
    p.add_argument("--out", default="enrichment.tsv", type=str, help=", ".join(HEADER) + " (default: enrichment.tsv)")
    p.add_argument("--null", default=None, type=str, help="also save the null scores [nodes][samples][sizes] as .npy (sizes = the distinct set sizes, ascending)")
    return p.parse_args(argv)


def check_args(nodes, min_size, max_size, samples, top):
    """every refusal that needs neither the graph nor the GPU"""
    if not nodes:
        raise PredictError("--node is missing: name at least one drug or indication")
    if len(set(nodes)) != len(nodes):
        raise PredictError(f"--node repeats a node in {nodes}")
    if min_size < 1:
        raise PredictError(f"--min-size {min_size} must be at least 1")
    if max_size > MAX_SET:
        raise PredictError(f"--max-size {max_size} is above {MAX_SET}, the most members a set is scored with")
    if max_size < min_size:
        raise PredictError(f"--max-size {max_size} is below --min-size {min_size}")
    if samples < 1:
        raise PredictError(f"--samples {samples} must be at least 1")
    if top is not None and top < 1:
        raise PredictError(f"--top {top} must be at least 1")


def read_gmt(path, place, err):
    """name<TAB>description<TAB>id ... per line -> [(name, description, [places, ascending])]; ids that are no universe node are dropped
    and counted on err"""
    sets, unknown = [], 0
    with open(path) as f:
        for line in f:
            cells = line.rstrip("\n").split("\t")
            if len(cells) < 2 or not cells[0]:
                continue
            ids = list(dict.fromkeys(c for c in cells[2:] if c))
            unknown += sum(1 for c in ids if c not in place)
            sets.append((cells[0], cells[1], sorted(place[c] for c in ids if c in place)))
    if unknown:
        print(f"enrich: dropped {unknown} ids of {path}: no protein node of the graph", file=err)
    return sets


def graph_sets(g, nodelist, kind, place):
    """the proteins adjacent to each node of type `kind`, in node order -> [(node, name, [places, ascending])]"""
    return [(n, g.node2name.get(n), sorted(place[v] for v in g.adj[n] if v in place)) for n in nodelist if g.type.get(n) == kind and n in g.adj]


def run(cfg_path, nodes, sets="functions", min_size=5, max_size=500, weighted=True, samples=1000, seed=0, top=None, out="enrichment.tsv",
        null=None, device="cuda", err=None):
    """the command -> (rows written, the number of sets scored)"""
    from .explain import check_profile
    err = sys.stderr if err is None else err
    nodes = list(nodes or [])
    check_args(nodes, min_size, max_size, samples, top)
    s = predict.Settings(predict.load_config(cfg_path))
    if not s.diffusion_dir:
        raise PredictError("config: diffusion.diffusion_embs_dir is missing")
    g = predict.build_graph(s)
    nodelist, profiles = predict.diffusion_profiles(s, g)
    for n in nodes:
        check_profile("--node", n, nodelist, profiles, g)
    universe = np.asarray([i for i, n in enumerate(nodelist) if g.type.get(n) == PROTEIN], dtype=np.int32)
    M = len(universe)
    if not 2 <= M <= MAX_UNIVERSE:
        raise PredictError(f"the graph has {M} protein nodes; the universe must hold 2 .. {MAX_UNIVERSE}")
    place = {nodelist[i]: u for u, i in enumerate(universe)}
    if sets in BUILT_IN_SETS:
        listed = graph_sets(g, nodelist, BUILT_IN_SETS[sets], place)
    else:
        listed = read_gmt(sets, place, err)
    upper = min(max_size, M - 1)      # a set of all M places has no random counterpart
    kept = [t for t in listed if min_size <= len(t[2]) <= upper]
    if not kept:
        raise PredictError(f"--sets {sets}: no set has {min_size} .. {upper} proteins in the universe of {M} ({len(listed)} sets read)")
    try:
        rec, _, null_host = enrichment(profiles, nodes, universe, [t[2] for t in kept], samples, seed, weighted, return_null=True, device=device)
    except ValueError as e:
        raise PredictError(str(e)) from None
    rows = []
    for j, node in enumerate(nodes):
        block = []
        for (name, label, _), r in zip(kept, rec[j * len(kept):(j + 1) * len(kept)]):
            if r["es"] != r["es"] and np.isnan(np.asarray(profiles[node], dtype=np.float64)[universe]).any():
                raise PredictError(f"the profile of {node!r} is NaN at a protein node; its sets cannot be scored")
            lead = [nodelist[universe[u]] for u in r["lead"]]
            block.append([node, g.node2name.get(node), name, label, r["size"], r["es"], r["nes"], r["p"], r["q"], len(lead), ",".join(lead)])
        block.sort(key=lambda b: (b[7] != b[7], b[7], -abs(b[6]) if b[6] == b[6] else float("inf"), b[2]))
        rows += block[:top]
    write_tsv(out, HEADER, rows)
    if null:
        np.save(null, null_host)
    return rows, len(kept)


def main(argv=None):
    a = parse_args(argv)
    try:
        check_args(a.node, a.min_size, a.max_size, a.samples, a.top)
        _, n_sets = run(a.config, a.node, a.sets, a.min_size, a.max_size, not a.unweighted, a.samples, a.seed, a.top, a.out, a.null)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"enrich: {e}", file=sys.stderr)
        sys.exit(2)
    print(f"enrichment: {len(a.node)} profiles x {n_sets} sets, {a.samples} samples, seed {a.seed}: {a.out}")
