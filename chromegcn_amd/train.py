"""Command-line entry of the GCN stage: what `python main.py ... -chrome_model gcn -adj_type hic ...`
(README.md:45, main.py:62-101) does after the window encoder's features have been saved -- build ChromeGCN,
optionally take the classifier head + BatchNorm affine from the pretrained CNN checkpoint (main.py:74-81), build the
optimizer (utils/util_methods.py:14-19) and run the epoch loop (runner.py:25-62) -- on the MI355X path.

    python -m chromegcn_amd.train -feat_dir <cnn_run_dir> -graph_root <graphs_dir> -hicsize 500000 -hicnorm SQRTVC \\
        -gcn_layers 2 -gcn_dropout 0.2 -optim sgd -lr 0.25 -epochs 1000 -model_name <out_dir> [-cnn_chkpt model.chkpt]

Inputs are the reference's own files: `<feat_dir>/chrom_feature_dict_{train,valid,test}.pt`
(utils/util_methods.py:183-199) and `<graph_root>/{split}_graphs_{hicsize}_{hicnorm}norm.pkl`
(data/7create_graph_new.py:197-202), or with `-hic_contacts DIR` the contact caches `DIR/<chrom>.cghic` from which the graphs
are built on the GPU for any `-hicsize` / `-hicnorm` (chromegcn_amd/hic.py).  `-synthetic` replaces them by the seeded GM12878-shaped stand-in.
`-hic_null distance|degree|uniform` replaces every Hi-C matrix, whatever its source, by its null graph (chromegcn_amd/nullgraph.py):
the control run that tells what the real contacts add.  `-hic_compartments RES_BP` (with `-hic_contacts`) calls every chromosome's A/B
compartments from its cache's records (chromegcn_amd/compartments.py), oriented by the split's label density, prints the A share, the
iteration's record and the AA / BB / AB share of the graph the run trains on, and after the last epoch the test metrics in A and in B;
`-hic_compartment_restrict` trains on the graphs of the contacts within one compartment.  `-hic_loops RES_BP` (with `-hic_contacts`) calls
every chromosome's chromatin loops from its cache's records (chromegcn_amd/loops.py) and prints the loop count and the share of the
unrestricted graph inside loop footprints; `-hic_loop_restrict` trains on the graphs of the contacts inside the footprints.
`-hic_apa W` (with `-hic_contacts`) prints the aggregate peak analysis (chromegcn_amd/pileup.py) of the unrestricted graph's edges,
of their shifted control and, with `-hic_loops`, of the loops; it changes no graph.  `-hic_compare DIR2` (with `-hic_contacts`) prints,
per chromosome, the stratum-adjusted correlation coefficient (chromegcn_amd/mapcompare.py) of the run's contact map and the map of
`DIR2/<chrom>.cghic`, and the overlap of the two unrestricted graphs' edges; it changes no graph either."""
from __future__ import annotations

import argparse
import os
import pickle
import sys
import time

import torch

from . import ChromeGCN, runner, synth


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-feat_dir", type=str, default=None)
    ap.add_argument("-graph_root", type=str, default=None)
    ap.add_argument("-hicsize", type=str, default="500000")          # config_args.py:47
    ap.add_argument("-hicnorm", type=str, default="SQRTVC")          # config_args.py:46
    ap.add_argument("-hic_contacts", type=str, default=None, metavar="DIR",
                    help="build every chromosome's graph on the GPU from DIR/<chrom>.cghic (chromegcn_amd.hic contact caches) "
                         "for the given -hicsize / -hicnorm, instead of opening a pickle under -graph_root")
    ap.add_argument("-hic_compute_norm", action="store_true",
                    help="-hic_contacts: compute a -hicnorm of KR / VC / SQRTVC that a cache lacks from its records on the GPU")
    ap.add_argument("-hic_upsample", action="store_true",
                    help="-hic_contacts: a cache whose records are coarser than -window_size (K562: 5 kb) stands for its "
                         "expanded file, every record for the window pairs it covers (data/extras/upsample_hic.py)")
    ap.add_argument("-hic_min_distance", type=int, default=0, metavar="BP",
                    help="-hic_contacts: keep a contact only if its two positions are at least BP apart "
                         "(data/7create_graph_old.py:167; the reference's graphs use 1000)")
    ap.add_argument("-hic_expected", action="store_true",
                    help="-hic_contacts: score a contact by observed / expected, the expected vector computed from the cache's "
                         "records on the GPU with the run's -hicnorm")
    ap.add_argument("-hic_domains", type=int, default=0, metavar="WINDOW_BP",
                    help="-hic_contacts: build every graph from the contacts that stay inside one domain, the domains found "
                         "from the cache's records by the insulation score at this window (chromegcn_amd.insulation; VC-balanced); "
                         "prints per chromosome the boundary count and the same-domain share of the unrestricted graph.  0: off")
    ap.add_argument("-hic_domain_res", type=int, default=10000, metavar="BP", help="-hic_domains: the bin size of the insulation score")
    ap.add_argument("-hic_domain_strength", type=float, default=0.5, metavar="X",
                    help="-hic_domains: the least boundary strength (log2 units)")
    ap.add_argument("-hic_compartments", type=int, default=0, metavar="RES_BP",
                    help="-hic_contacts: call every chromosome's A/B compartments at this bin size from the cache's records "
                         "(chromegcn_amd.compartments), oriented by the split's label density; prints per chromosome the A share of "
                         "the called bins, the eigenvector iteration's record and the AA / BB / AB share of the graph, and after "
                         "the last epoch the means of the test metrics in A and in B.  0: off")
    ap.add_argument("-hic_compartment_norm", type=str, default="VC", choices=["KR", "VC", "SQRTVC", "NONE"],
                    help="-hic_compartments: the balancing of the map the compartments are called on")
    ap.add_argument("-hic_compartment_restrict", action="store_true",
                    help="-hic_compartments: build every graph from the contacts within one compartment")
    ap.add_argument("-hic_loops", type=int, default=0, metavar="RES_BP",
                    help="-hic_contacts: call every chromosome's chromatin loops at this bin size (5000, 10000 or 25000) from the "
                         "cache's records (chromegcn_amd.loops); prints per chromosome the loop count and the share of the "
                         "unrestricted graph inside loop footprints.  0: off")
    ap.add_argument("-hic_loop_norm", type=str, default="VC", choices=["KR", "VC", "SQRTVC", "NONE"],
                    help="-hic_loops: the balancing of the map the loops are called on")
    ap.add_argument("-hic_loop_fdr", type=float, default=0.1, metavar="Q", help="-hic_loops: the false discovery rate of the thresholds")
    ap.add_argument("-hic_loop_pad", type=int, default=1, metavar="BINS", help="-hic_loops: a footprint reaches this far around a peak")
    ap.add_argument("-hic_loop_restrict", action="store_true",
                    help="-hic_loops: build every graph from the contacts inside loop footprints")
    ap.add_argument("-hic_apa", type=int, default=0, metavar="W",
                    help="-hic_contacts: pile the observed / expected map up in a (2 W + 1)^2 window (chromegcn_amd.pileup) around the "
                         "edges of every chromosome's unrestricted graph, around the same edges shifted by 3 W bins and, with "
                         "-hic_loops, around the loops; prints P2LL, P2M and ZscoreLL of each.  0: off")
    ap.add_argument("-hic_apa_res", type=int, default=10000, metavar="BP", help="-hic_apa: the bin size of the piled-up map")
    ap.add_argument("-hic_compare", type=str, default=None, metavar="DIR2",
                    help="-hic_contacts: compare every chromosome's contact map with DIR2/<chrom>.cghic (chromegcn_amd.mapcompare); "
                         "prints the stratum-adjusted correlation coefficient of the two maps and the overlap of the two "
                         "unrestricted graphs' edges")
    ap.add_argument("-hic_compare_res", type=int, default=40000, metavar="BP", help="-hic_compare: the bin size of the compared maps")
    ap.add_argument("-hic_compare_h", type=int, default=5, metavar="H", help="-hic_compare: the smoothing half-width, 0 to 20 bins")
    ap.add_argument("-hic_compare_norm", type=str, default="NONE", choices=["KR", "VC", "SQRTVC", "NONE"],
                    help="-hic_compare: the balancing of the compared maps (NONE: the observed counts)")
    ap.add_argument("-hic_null", type=str, default=None, choices=["distance", "degree", "uniform"],
                    help="the control the reference's `-adj_type random` advertises: every Hi-C matrix of every split is replaced "
                         "by its null graph (chromegcn_amd.nullgraph) before it is normalised by -adj_type hic / both")
    ap.add_argument("-hic_null_seed", type=int, default=0,
                    help="-hic_null: chromosome index c of a split's K chromosomes draws with seed + c")
    ap.add_argument("-window_size", type=int, default=1000)          # config_args.py:9
    ap.add_argument("-adj_type", type=str, default="hic", choices=["constant", "hic", "both", "none"])
    ap.add_argument("-gcn_layers", type=int, default=2)              # config_args.py:40
    ap.add_argument("-gcn_dropout", type=float, default=0.2)         # config_args.py:24
    ap.add_argument("-gate", action="store_true")                    # accepted, ignored (ChromeModels.py:22-31)
    ap.add_argument("-optim", type=str, default="sgd", choices=["adam", "sgd"])
    ap.add_argument("-fused_adam", action="store_true",
                    help="-optim adam: build Adam(fused=True), whose step runs as one HIP launch inside the captured graphs "
                         "(off: torch's default Adam, stepped eagerly after each captured forward + backward)")
    ap.add_argument("-lr", type=float, default=0.25)
    ap.add_argument("-lr_decay2", type=float, default=0)
    ap.add_argument("-epochs", type=int, default=100)
    ap.add_argument("-model_name", type=str, default="results/gcn_run")
    ap.add_argument("-cnn_chkpt", type=str, default=None, help="pretrained window-model checkpoint (main.py:74-81)")
    ap.add_argument("-load_gcn", type=str, default=None, help="ChromeGCN checkpoint to evaluate (main.py:66-69)")
    ap.add_argument("-synthetic", action="store_true")
    ap.add_argument("-synthetic_chroms", type=str, default=",".join(synth.HG19_LEN))
    ap.add_argument("-gpu_id", type=int, default=0)
    ap.add_argument("-br_threshold", type=float, default=None,       # config_args.py:28 (there 0.5; here off unless given)
                    help="also report ACC, HA, ebF1, miF1, maF1 of the decisions p >= this (chromegcn_amd.thresholds)")
    ap.add_argument("-bootstrap", type=int, default=0, metavar="B",
                    help="after the last epoch, print 95 %% block-bootstrap intervals of the test split's mAP, meanAUC, meanAUPR and "
                         "meanFDR from B replicates, the test chromosomes as strata (chromegcn_amd.bootstrap)")
    ap.add_argument("-bootstrap_block", type=int, default=50, metavar="L", help="-bootstrap: block length in windows")
    ap.add_argument("-summarize_data", action="store_true",     # config_args.py:35
                    help="print labels per window and windows per label (mean, median, max) of train + valid before the "
                         "first epoch (utils/util_methods.py:64-74; chromegcn_amd.labelstats)")
    opt = ap.parse_args(argv)
    if opt.hic_apa:
        if not opt.hic_contacts:
            ap.error("-hic_apa needs -hic_contacts: the pile-up reads the contact records")
        if not 1 <= opt.hic_apa <= 10:
            ap.error("-hic_apa: the window half-width is 1 to 10 bins")
        if opt.hic_apa_res < 1:
            ap.error("-hic_apa_res must be positive")
    if opt.hic_compare:
        if not opt.hic_contacts:
            ap.error("-hic_compare needs -hic_contacts: the comparison reads the contact records of both directories")
        if not 0 <= opt.hic_compare_h <= 20:
            ap.error("-hic_compare_h: the smoothing half-width is 0 to 20 bins")
        if opt.hic_compare_res < 1:
            ap.error("-hic_compare_res must be positive")
    return opt


def report_compare(split, report, out=None):
    """-hic_compare: one line per chromosome of graphs_from_contact_caches' compare_report"""
    for c, (cmp, ov) in report.items():
        print("[hic_compare] %s %s: SCC %.4f, N strata %d, edges shared/only/only %d/%d/%d, Jaccard %.4f"
              % (split, c, cmp.scc, cmp.n_strata, ov["shared"], ov["only_a"], ov["only_b"], ov["jaccard"]), file=out)


def report_apa(split, report, out=None):
    """-hic_apa: P2LL, P2M and ZscoreLL per chromosome and centre set of graphs_from_contact_caches' apa_report"""
    for c, piles in report.items():
        for name, p in piles.items():
            s = p.scores()
            print("[hic_apa] %s %s %s: %d centres kept (%d skipped), P2LL %.4g, P2M %.4g, ZscoreLL %.4g"
                  % (split, c, name, int(p.kept[0]), sum(p.skipped.values()), s["P2LL"][0], s["P2M"][0], s["ZscoreLL"][0]), file=out)


def summarize_data(data, dev, out=None):
    """The six numbers of the reference's summarize_data (utils/util_methods.py:64-74) for train + valid, counted on the
    device (chromegcn_amd.labelstats); returns the pooled LabelStats."""
    from . import labelstats
    targets = [f["target"].to(dev) for sp in ("train", "valid") for f in data[sp].values()]
    stats = labelstats.label_stats_split(targets)
    lw, sl = stats.labels_per_window(), stats.samples_per_label()
    for text, v in (("Mean Labels Per Sample", lw["mean"]), ("Median Labels Per Sample", lw["median"]),
                    ("Max Labels Per Sample", lw["max"]), ("Mean Samples Per Label", sl["mean"]),
                    ("Median Samples Per Label", sl["median"]), ("Max Samples Per Label", sl["max"])):
        print("%s: %s" % (text, round(v, 4)), file=out)
    return stats


def null_graphs(graphs, opt, dev):
    """-hic_null: {chrom: matrix} of one split -> {chrom: ChromGraph of the null graph, normalised by opt.adj_type}; the
    chromosome at index c of the K in the split draws with nullgraph.replicate_seed(opt.hic_null_seed, 0, c, K)"""
    from . import nullgraph
    seed, K = getattr(opt, "hic_null_seed", 0), len(graphs)
    return {c: nullgraph.null_chrom_graph(a, opt.adj_type, opt.hic_null, nullgraph.replicate_seed(seed, 0, i, K), device=dev)
            for i, (c, a) in enumerate(graphs.items())}


def report_compartments(opt, split, report, out=None):
    """-hic_compartments: one line per chromosome of graphs_from_contact_caches' compartment_report, and the calls of the split's
    windows in the order of its chromosomes kept in opt.compartment_of_window[split] for the metrics after the last epoch"""
    import numpy as np
    for c, (comp, _, share) in report.items():
        info = {k: v[0] for k, v in comp.info.items() if isinstance(v, list)}
        print("[hic_compartments] %s %s: %d of %d bins called, A share %.3f; converged %s after %d steps, eigenvalue %.4g, "
              "residual %.2e, %d flat rows; graph entries AA %d BB %d AB %d uncalled %d of %d (%.1f / %.1f / %.1f %%)"
              % (split, c, int(np.count_nonzero(comp.compartment_of_bin)), comp.n, comp.a_share(), info["converged"],
                 info["iterations"], info["eigenvalue"], info["residual"], comp.info["flat_rows"], share["AA"], share["BB"],
                 share["AB"], share["uncalled"], share["nnz"], 100.0 * share["AA"] / max(share["nnz"], 1),
                 100.0 * share["BB"] / max(share["nnz"], 1), 100.0 * share["AB"] / max(share["nnz"], 1)), file=out)
    if report:
        if not hasattr(opt, "compartment_of_window"):
            opt.compartment_of_window = {}
        opt.compartment_of_window[split] = np.concatenate([cw for _, cw, _ in report.values()])


def load_inputs(opt):
    data, graphs = _load_inputs(opt)
    if getattr(opt, "hic_null", None) and opt.adj_type in ("hic", "both") and not opt.hic_contacts:
        dev = torch.device("cuda", opt.gpu_id)   # (contact caches: graphs_from_contact_caches has done it, before the band)
        graphs = {sp: null_graphs(g, opt, dev) if g else g for sp, g in graphs.items()}
    return data, graphs


def _load_inputs(opt):
    data, graphs = {}, {}
    if opt.synthetic:
        for sp in ("train", "valid", "test"):
            data[sp], graphs[sp] = {}, {}
        for c in opt.synthetic_chroms.split(","):
            feats, hic = synth.synthetic_chromosome(c)
            data[synth.split_of(c)][c] = feats
            graphs[synth.split_of(c)][c] = hic
        return data, graphs
    if not opt.feat_dir:
        raise SystemExit("-feat_dir is required (or -synthetic)")
    for sp in ("train", "valid", "test"):
        data[sp] = torch.load(os.path.join(opt.feat_dir, "chrom_feature_dict_%s.pt" % sp), map_location="cpu")   # main.py:30-32
        graphs[sp] = None
        if opt.adj_type in ("hic", "both") and opt.hic_contacts:
            from . import hic
            domains, report = None, {}
            if getattr(opt, "hic_domains", 0):
                domains = dict(window_bp=opt.hic_domains, resolution_bp=opt.hic_domain_res, min_strength=opt.hic_domain_strength)
            comps, comp_report = None, {}
            if getattr(opt, "hic_compartments", 0):
                comps = dict(resolution_bp=opt.hic_compartments, restrict=bool(opt.hic_compartment_restrict),
                             norm=None if opt.hic_compartment_norm == "NONE" else opt.hic_compartment_norm,
                             targets={c: f["target"] for c, f in data[sp].items()})
            loops, loop_report = None, {}
            if getattr(opt, "hic_loops", 0):
                loops = dict(resolution_bp=opt.hic_loops, norm=None if opt.hic_loop_norm == "NONE" else opt.hic_loop_norm,
                             fdr=opt.hic_loop_fdr, pad_bins=opt.hic_loop_pad, restrict=bool(opt.hic_loop_restrict))
            apa = {}
            if getattr(opt, "hic_apa", 0):
                apa = dict(apa=dict(w=opt.hic_apa, resolution_bp=opt.hic_apa_res), apa_report={})
            if getattr(opt, "hic_compare", None):
                apa.update(compare=dict(root=opt.hic_compare, resolution_bp=opt.hic_compare_res, h=opt.hic_compare_h,
                                        norm=None if opt.hic_compare_norm == "NONE" else opt.hic_compare_norm),
                           compare_report={})
            graphs[sp] = hic.graphs_from_contact_caches(opt.hic_contacts, list(data[sp]), opt.hicsize, opt.hicnorm, opt.adj_type,
                                                        torch.device("cuda", opt.gpu_id),
                                                        {c: f["forward"].shape[0] for c, f in data[sp].items()},
                                                        window_bp=opt.window_size if opt.hic_upsample else None,
                                                        compute_norm=opt.hic_compute_norm,
                                                        min_distance_bp=opt.hic_min_distance,
                                                        expected="auto" if opt.hic_expected else None,
                                                        null=((opt.hic_null, getattr(opt, "hic_null_seed", 0))
                                                              if getattr(opt, "hic_null", None) else None),
                                                        domains=domains, domain_report=report,
                                                        compartments=comps, compartment_report=comp_report,
                                                        loops=loops, loop_report=loop_report, **apa)
            report_compartments(opt, sp, comp_report)
            report_apa(sp, apa.get("apa_report", {}))
            report_compare(sp, apa.get("compare_report", {}))
            for c, (called, inside, nnz) in loop_report.items():
                print("[hic_loops] %s %s: %d loops from %d candidates (%d enriched pixels, %d after the ratios); %d of %d entries of the "
                      "unrestricted graph inside a footprint (%.1f %%)"
                      % (sp, c, len(called), called.info["candidates"], called.info["enriched"], called.info["kept_after_ratios"],
                         inside, nnz, 100.0 * inside / max(nnz, 1)))
            for c, (n_bound, same, nnz) in report.items():
                print("[hic_domains] %s %s: %d boundaries, %d of %d entries of the unrestricted graph inside a domain (%.1f %%)"
                      % (sp, c, n_bound, same, nnz, 100.0 * same / max(nnz, 1)))
        elif opt.adj_type in ("hic", "both"):
            path = os.path.join(opt.graph_root, sp + "_graphs_" + opt.hicsize + "_" + opt.hicnorm + "norm.pkl")  # finetune.py:21
            with open(path, "rb") as f:
                graphs[sp] = pickle.load(f)
    return data, graphs


def main(argv=None):
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("chromegcn_amd.train needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(opt.gpu_id)
    dev = torch.device("cuda", opt.gpu_id)
    data, graphs = load_inputs(opt)
    if opt.summarize_data:
        summarize_data(data, dev)
    first = next(iter(data["train"].values())) if data["train"] else next(iter(data["test"].values()))
    d, n_class = first["forward"].shape[1], first["target"].shape[1]
    model = ChromeGCN(d, d, n_class, opt.gcn_dropout, opt.gate, opt.gcn_layers)       # main.py:62
    if opt.load_gcn:
        ck = torch.load(opt.load_gcn, map_location="cpu", weights_only=False)
        model.load_state_dict(ck["model"])                                           # main.py:66-69
    elif opt.cnn_chkpt:
        sd = torch.load(opt.cnn_chkpt, map_location="cpu", weights_only=False)["model"]
        pick = lambda suffix: next(v for k, v in sd.items() if k.endswith(suffix))   # DataParallel prefixes (main.py:75)
        with torch.no_grad():                                                        # main.py:78-81
            model.out.weight.copy_(pick("model.classifier.weight")); model.out.bias.copy_(pick("model.classifier.bias"))
            model.batch_norm.weight.copy_(pick("model.batch_norm.weight")); model.batch_norm.bias.copy_(pick("model.batch_norm.bias"))
    model.to(dev)
    if opt.optim == "adam":                                                          # utils/util_methods.py:14-19
        optimizer = torch.optim.Adam(model.parameters(), betas=(0.9, 0.98), lr=opt.lr, fused=bool(opt.fused_adam) or None)
    else:
        optimizer = torch.optim.SGD(model.parameters(), lr=opt.lr, weight_decay=1e-6, momentum=0.9)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=100, gamma=0.5)  # main.py:86
    opt.test_only = bool(opt.load_gcn)
    opt.load_gcn = bool(opt.load_gcn)
    t0 = time.time()
    hist = runner.run_model(None, model, data["train"], data["valid"], data["test"], None, optimizer, scheduler, opt, None,
                            graphs=graphs)
    print("done: %d epochs in %.2f s -> %s" % (len(hist), time.time() - t0, opt.model_name))
    return hist


if __name__ == "__main__":
    main(sys.argv[1:])
