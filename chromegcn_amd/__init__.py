"""chromegcn_amd -- MI355X-native gated graph-convolution hot path of ChromeGCN.

Public surface mirrors the reference modules it replaces (see layers.py / graph.py / finetune.py)."""
from .ablation import label_pair_ablation  # noqa: F401
from .curves import (Curves, optimal_cutoff_host, optimal_cutoffs, pr_curve_host, pr_curves, roc_curve_host,  # noqa: F401
                     roc_curves)
from .effects import (WindowEffects, effect_rows_host, knockout_map, knockout_map_host, window_effects,  # noqa: F401
                      window_effects_host)
from .embed import class_embeddings  # noqa: F401
from .graph import ChromGraph, HostCSR, normalize_graph, process_graph, upload, as_graph  # noqa: F401
from .bootstrap import (BootstrapComparison, BootstrapResult, bootstrap_compare, bootstrap_metrics,  # noqa: F401
                        bootstrap_summary, bootstrap_weights, bootstrap_weights_host, metrics_from_sums, weighted_metrics,
                        weighted_sums, weighted_sums_host)
from .compare import compare_labels  # noqa: F401
from .compartments import (Compartments, compartment_edge_share, compartment_metrics, compartments_host,  # noqa: F401
                           compartments_of_matrix, label_density)
from .handoff import FeatureCollector  # noqa: F401
from .hic import (HicContacts, build_hic_graph, build_hic_graph_host, contacts_from_text, expand_contacts_host,  # noqa: F401
                  parse_contacts_text_host, release_text_staging, windows_from_bed)
from .hicnorm import (HicNormError, contact_matrix_host, hic_norm_vector, hic_norm_vector_host,  # noqa: F401
                      kr_balance_host)
from .hicdist import (distance_sums_device_order_host, distance_sums_host, expected_from_sums, expected_vector_host,  # noqa: F401
                      hic_expected_vector)
from .hicmap import device_band  # noqa: F401
from .insulation import (Insulation, diamond_sums, diamond_sums_host, domain_edge_share, domain_of_windows,  # noqa: F401
                         insulation_from_sums, insulation_host)
from .loops import (Loops, chunk_boundaries, enriched_pixels, enriched_pixels_host, loop_edge_share,  # noqa: F401
                    loop_histograms, loop_histograms_host, loop_lambdas_host, loop_thresholds, loops_from_pixels, loops_host,
                    loops_of_matrix, neighbourhood_offsets, same_loop_host)
from .pileup import (Pileup, PileupRule, apa_scores, centres_of_graph, distance_groups, pileup_host,  # noqa: F401
                     pileup_of_matrix, pileup_rule, pileup_sums, pileup_sums_host, quantile_groups, shifted_centres,
                     value_band, value_band_host)
from .mapcompare import (MapComparison, SccRule, graph_edge_overlap, map_scc, map_scc_host, scc_from_sums,  # noqa: F401
                         scc_rule, smooth_strata, smooth_strata_host, stratum_sums, stratum_sums_host)
from .labelstats import LabelStats, label_stats, label_stats_host, label_stats_split  # noqa: F401
from .nullgraph import (NullGraphTest, null_chrom_graph, null_graph, null_graph_host, null_graph_test,  # noqa: F401
                        null_statistics)
from .pairs import ReadPairs, bin_read_pairs_host, pairs_to_contacts_host  # noqa: F401
from .layers import ChromeGCN, GraphConvolution  # noqa: F401
from .thresholds import (ThresholdCounts, best_thresholds, metrics_from_counts, threshold_counts,  # noqa: F401
                         threshold_counts_host, threshold_metrics, threshold_metrics_host)
from .tsne import (TsneAffinities, joint_probabilities_host, kl_gradient_host, tsne_embed, tsne_embed_host,  # noqa: F401
                   tsne_sweep)

__all__ = ["ChromeGCN", "GraphConvolution", "ChromGraph", "HostCSR", "normalize_graph", "process_graph",
           "upload", "as_graph", "FeatureCollector", "label_pair_ablation", "HicContacts",
           "build_hic_graph", "build_hic_graph_host", "expand_contacts_host", "contacts_from_text",
           "parse_contacts_text_host", "release_text_staging", "windows_from_bed", "class_embeddings",
           "TsneAffinities", "tsne_embed", "tsne_sweep", "joint_probabilities_host",
           "kl_gradient_host", "tsne_embed_host", "Curves", "roc_curves", "pr_curves", "optimal_cutoffs",
           "roc_curve_host", "pr_curve_host", "optimal_cutoff_host", "ThresholdCounts", "threshold_counts",
           "threshold_metrics", "metrics_from_counts", "best_thresholds", "threshold_counts_host",
           "threshold_metrics_host", "HicNormError", "contact_matrix_host", "kr_balance_host",
           "hic_norm_vector_host", "hic_norm_vector", "distance_sums_host", "expected_from_sums",
           "expected_vector_host", "hic_expected_vector", "ReadPairs", "bin_read_pairs_host", "pairs_to_contacts_host",
           "LabelStats", "label_stats", "label_stats_split", "label_stats_host", "compare_labels",
           "WindowEffects", "window_effects", "window_effects_host", "effect_rows_host", "knockout_map", "knockout_map_host",
           "NullGraphTest", "null_graph", "null_graph_host", "null_chrom_graph", "null_graph_test", "null_statistics",
           "BootstrapResult", "BootstrapComparison", "bootstrap_weights_host", "bootstrap_weights", "weighted_sums_host",
           "weighted_sums", "metrics_from_sums", "weighted_metrics", "bootstrap_metrics", "bootstrap_compare",
           "bootstrap_summary", "Insulation", "diamond_sums", "diamond_sums_host", "insulation_from_sums", "insulation_host",
           "domain_edge_share", "domain_of_windows", "Compartments", "compartments_host", "compartments_of_matrix",
           "compartment_edge_share", "compartment_metrics", "label_density", "Loops", "neighbourhood_offsets",
           "chunk_boundaries", "loop_thresholds", "loops_from_pixels", "loop_lambdas_host", "loop_histograms_host",
           "enriched_pixels_host", "loops_host", "device_band", "loop_histograms", "enriched_pixels", "loops_of_matrix",
           "same_loop_host", "loop_edge_share", "Pileup", "PileupRule", "pileup_rule", "apa_scores", "value_band_host",
           "pileup_sums_host", "pileup_host", "value_band", "pileup_sums", "pileup_of_matrix", "centres_of_graph",
           "shifted_centres", "distance_groups", "quantile_groups", "MapComparison", "SccRule", "scc_rule", "scc_from_sums",
           "smooth_strata_host", "stratum_sums_host", "map_scc_host", "smooth_strata", "stratum_sums", "map_scc",
           "graph_edge_overlap"]
