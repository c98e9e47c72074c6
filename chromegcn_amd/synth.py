"""Seeded synthetic stand-ins for the data the hot path consumes (the real GM12878/K562 files need
a 13 GB download, README.md:16-21).  Shapes follow SURVEY.md section 8(d) / Appendix C:

  * graphs: symmetric {0,1} float64 CSR with zero diagonal -- the on-disk contract of
    data/7create_graph_new.py:108-120 -- with `pairs` undirected contact pairs per chromosome
    (hic_edges/2, data/create_data.py:27, data/7create_graph_new.py:168);
  * node features / targets: the chrom_feature_dict contract of utils/util_methods.py:183-199."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import scipy.sparse as sp
import torch

# hg19 autosome lengths (UCSC hg19.chrom.sizes; the reference reads the same file, data/create_data.py:32)
HG19_LEN = {
    "chr1": 249250621, "chr2": 243199373, "chr3": 198022430, "chr4": 191154276, "chr5": 180915260,
    "chr6": 171115067, "chr7": 159138663, "chr8": 146364022, "chr9": 141213431, "chr10": 135534747,
    "chr11": 135006516, "chr12": 133851895, "chr13": 115169878, "chr14": 107349540, "chr15": 102531392,
    "chr16": 90354753, "chr17": 81195210, "chr18": 78077248, "chr19": 59128983, "chr20": 63025520,
    "chr21": 48129895, "chr22": 51304566,
}
VALID_CHROMS = ["chr3", "chr12", "chr17"]  # data/create_data.py:44
TEST_CHROMS = ["chr1", "chr8", "chr21"]    # data/create_data.py:45
PEAK_FRACTION = 0.12   # assumed share of 1 kb windows overlapping a peak
PAIRS_PER_CHROM = 250000  # -hicsize 500000 => 250k undirected pairs (README.md:45)
N_LABELS = 103         # assumed label count (data dependent in the reference, main.py:35)


def chrom_nodes(chrom: str, fraction: float = PEAK_FRACTION) -> int:
    return int(round(fraction * HG19_LEN[chrom] / 1000.0))


def split_of(chrom: str) -> str:
    return "valid" if chrom in VALID_CHROMS else "test" if chrom in TEST_CHROMS else "train"


def chrom_seed(chrom: str) -> int:
    return int(chrom[3:])


GENERATORS = ("uniform", "hic_like", "hub")


def contact_graph(n: int, pairs: int, seed: int, hic_like=False) -> sp.csr_matrix:
    """`pairs` undirected contact pairs on n windows.  hic_like: False / "uniform" = uniform-random pairs; True /
    "hic_like" = pairs whose genomic distance |i-j| follows a truncated 1/k law, so contacts concentrate near the
    diagonal like real Hi-C; "hub" = a top-K-style graph: the reference keeps the `hic_edges/2` HIGHEST-scoring pairs of
    a chromosome (data/7create_graph_new.py:93-104), and normalised contact scores are dominated by a few
    high-coverage bins, so the kept edges pile up on them -- a heavy-tailed degree distribution with hubs of thousands
    of neighbours.  Modelled as: 8 hubs with 2 000 ... min(10 000, n/2) neighbours each (uniform random partners),
    the rest of the budget drawn with power-law endpoint propensities (w_i ~ rank^-0.6, random rank order) -- degrees
    from 1 to 10^4 on the same edge budget as the other generators."""
    kind = hic_like if isinstance(hic_like, str) else ("hic_like" if hic_like else "uniform")
    if kind not in GENERATORS:
        raise ValueError("unknown contact generator %r" % (kind,))
    rng = np.random.RandomState(seed)
    if kind == "hic_like":
        kmax = max(2, n - 1)
        u = rng.random_sample(pairs)
        dist = np.clip(np.floor(np.exp(u * math.log(kmax))).astype(np.int64), 1, n - 1)
        i = (rng.random_sample(pairs) * (n - dist)).astype(np.int64)
        j = i + dist
    elif kind == "hub":
        n_hubs = min(8, max(1, n // 64))
        hubs = rng.choice(n, n_hubs, replace=False)
        hi_deg = max(2, min(10000, n // 2))
        lo_deg = max(1, min(2000, hi_deg // 2))
        ii, jj = [], []
        for h in hubs:
            deg = int(rng.randint(lo_deg, hi_deg + 1))
            nb = rng.choice(n, deg, replace=False)
            ii.append(np.full(deg, h, dtype=np.int64))
            jj.append(nb.astype(np.int64))
        used = sum(a.size for a in ii)
        rest = max(0, pairs - used)
        w = np.arange(1, n + 1, dtype=np.float64) ** -0.6
        w = w[rng.permutation(n)]
        w /= w.sum()
        ii.append(rng.choice(n, rest, p=w).astype(np.int64))
        jj.append(rng.choice(n, rest, p=w).astype(np.int64))
        i, j = np.concatenate(ii), np.concatenate(jj)
    else:
        i = rng.randint(0, n, pairs)
        j = rng.randint(0, n, pairs)
    keep = i != j
    i, j = i[keep], j[keep]
    a = sp.coo_matrix((np.ones(i.size), (i, j)), shape=(n, n)).tocsr()
    a = a + a.T
    a.data[:] = 1.0
    a.sort_indices()
    return sp.csr_matrix(a, dtype=np.float64)


def raw_contacts(chrom: str, seed: int = None, resolution_bp: int = 1000, background_per_bin: float = 80.0,
                 peak_pairs_per_window: float = 120.0) -> dict:
    """Seeded synthetic contact records at a real chromosome's shape, in the form chromegcn_amd.hic consumes: what a
    `RAWobserved` file plus a norm file plus the window list of data/7create_graph_new.py hold.
      * every `resolution_bp` bin of the chromosome exists; a PEAK_FRACTION share of them (chrom_nodes) are windows with
        peaks: `window_start`, strictly increasing;
      * records sorted by (pos1, pos2), pos1 <= pos2, each ordered pair once, like the real files; the distance of a pair
        follows the truncated 1/k law of contact_graph(hic_like=True);
      * `background_per_bin` x bins records between any two bins (1.4 % of them survive the window filter) and
        `peak_pairs_per_window` x windows drawn with BOTH ends on windows, so that the survivors outnumber the 250 000
        pairs of the default budget and the top-K cut binds;
      * integer counts that fall with distance (1 + Poisson: heavy ties, as in raw counts); a norm vector around 1 with
        2 % NaN and 1 % zero entries.
    Returns {'pos1', 'pos2' int32 [M], 'count' float64 [M], 'norm' float64 [n_bins], 'window_start' int32 [N],
    'resolution_bp'}."""
    rng = np.random.RandomState(chrom_seed(chrom) + 7000 if seed is None else seed)
    n_bins = -(-HG19_LEN[chrom] // resolution_bp)
    n = min(chrom_nodes(chrom), n_bins)
    windows = np.sort(rng.choice(n_bins, n, replace=False)).astype(np.int64)

    def pairs(count, size):   # (a, b), a < b < size, b - a from the truncated 1/k law
        dist = np.clip(np.floor(np.exp(rng.random_sample(count) * math.log(max(2, size - 1)))).astype(np.int64), 1, size - 1)
        a = (rng.random_sample(count) * (size - dist)).astype(np.int64)
        return a, a + dist

    a0, b0 = pairs(int(background_per_bin * n_bins), n_bins)
    a1, b1 = pairs(int(peak_pairs_per_window * n), n)
    diag = rng.randint(0, n_bins, n_bins // 8)   # pos1 == pos2 records: real files have the diagonal, the rule drops it
    b1p = np.concatenate([a0, windows[a1], diag])
    b2p = np.concatenate([b0, windows[b1], diag])
    key = np.unique(b1p * n_bins + b2p)   # each ordered pair once, sorted by (pos1, pos2)
    bin1, bin2 = key // n_bins, key % n_bins
    count = 1.0 + rng.poisson(40.0 / (1.0 + (bin2 - bin1)) ** 0.8)
    norm = 0.5 + rng.random_sample(n_bins)
    norm[rng.random_sample(n_bins) < 0.02] = np.nan
    norm[rng.random_sample(n_bins) < 0.01] = 0.0
    return {"pos1": (bin1 * resolution_bp).astype(np.int32), "pos2": (bin2 * resolution_bp).astype(np.int32),
            "count": count.astype(np.float64), "norm": norm, "window_start": (windows * resolution_bp).astype(np.int32),
            "resolution_bp": int(resolution_bp)}


def raw_contacts_coarse(chrom: str, resolution_bp: int = 5000, window_bp: int = 1000, seed: int = None, **kw) -> dict:
    """raw_contacts(chrom, resolution_bp=window_bp, ...) as a coarser experiment records it (K562: 5 kb records for 1 kb
    windows): the same distance-decay contacts binned to `resolution_bp`, counts summed, records sorted by (pos1, pos2), upper
    triangle, diagonal records present; a norm vector of its own at `resolution_bp`; the windows stay at `window_bp`.
    Returns raw_contacts' dict plus 'window_bp'."""
    if resolution_bp % window_bp:
        raise ValueError("window_bp must divide resolution_bp")
    r = raw_contacts(chrom, seed=seed, resolution_bp=window_bp, **kw)
    n_bins = -(-HG19_LEN[chrom] // resolution_bp)
    key = (r["pos1"].astype(np.int64) // resolution_bp) * n_bins + r["pos2"].astype(np.int64) // resolution_bp
    key, inv = np.unique(key, return_inverse=True)
    count = np.bincount(inv.reshape(-1), weights=r["count"], minlength=key.size)
    rng = np.random.RandomState((chrom_seed(chrom) if seed is None else seed) + 9000)
    norm = 0.5 + rng.random_sample(n_bins)
    norm[rng.random_sample(n_bins) < 0.02] = np.nan
    norm[rng.random_sample(n_bins) < 0.01] = 0.0
    return {"pos1": (key // n_bins * resolution_bp).astype(np.int32), "pos2": (key % n_bins * resolution_bp).astype(np.int32),
            "count": count.astype(np.float64), "norm": norm, "window_start": r["window_start"],
            "resolution_bp": int(resolution_bp), "window_bp": int(window_bp)}


def read_pairs(chrom_sizes: Dict[str, int], n_pairs: int, seed: int, inter_share: float = 0.15, duplicate_share: float = 0.2,
               name_prefix: str = "SRR5831489") -> bytes:
    """The text of a HiC-Pro-shaped `allValidPairs` file of `n_pairs` lines over the chromosomes of `chrom_sizes` (name ->
    length in bp): 12 TAB-separated columns -- read name, chr1, pos1, strand1, chr2, pos2, strand2, fragment size, two
    restriction-fragment names and two mapping qualities -- with read names of varying length, an `inter_share` of
    inter-chromosomal pairs, separations that follow the truncated 1/k law of contact_graph(hic_like=True) (down to a few bp, so
    that some pairs fall into one bin), and a `duplicate_share` of lines that repeat an earlier pair's two positions under a
    new read name.  Pairs are spread over the chromosomes by length; the second read is the upstream one in half of them.
    Seeded: the same arguments give the same bytes."""
    rng = np.random.RandomState(seed)
    names = list(chrom_sizes)
    sizes = np.array([chrom_sizes[c] for c in names], dtype=np.int64)
    n = int(n_pairs)
    c1 = rng.choice(len(names), n, p=sizes / sizes.sum())
    size = sizes[c1]
    dist = np.minimum(np.floor(np.exp(rng.random_sample(n) * np.log(size - 1.0))).astype(np.int64), size - 1)
    a = (rng.random_sample(n) * (size - dist)).astype(np.int64)
    b = a + dist
    dup = np.flatnonzero(rng.random_sample(n) < duplicate_share)
    dup = dup[dup > 0]
    src = (rng.random_sample(dup.size) * dup).astype(np.int64)   # an earlier line (which may itself be a copy further down)
    order = np.argsort(dup)
    for d, s in zip(dup[order].tolist(), src[order].tolist()):
        c1[d], a[d], b[d] = c1[s], a[s], b[s]
    c2 = c1.copy()
    if len(names) > 1:
        inter = np.flatnonzero(rng.random_sample(n) < inter_share)
        c2[inter] = (c1[inter] + 1 + rng.randint(0, len(names) - 1, inter.size)) % len(names)
        b[inter] = (rng.random_sample(inter.size) * sizes[c2[inter]]).astype(np.int64)
    swap = rng.random_sample(n) < 0.5
    a, b = np.where(swap & (c1 == c2), b, a), np.where(swap & (c1 == c2), a, b)
    cols = [("%s.%%d" % name_prefix) % k for k in range(1, n + 1)]
    for extra in (rng.randint(1101, 2679, n), rng.randint(1000, 30000, n), rng.randint(1000, 200000, n)):
        cols = [c + ":" + e for c, e in zip(cols, map(str, extra.tolist()))]   # read names of varying length
    s1, s2 = rng.randint(0, 2, n).tolist(), rng.randint(0, 2, n).tolist()
    n1, n2 = [names[k] for k in c1.tolist()], [names[k] for k in c2.tolist()]
    rows = zip(cols, n1, map(str, a.tolist()), ("+-"[k] for k in s1), n2, map(str, b.tolist()), ("+-"[k] for k in s2),
               map(str, rng.randint(50, 900, n).tolist()),
               ("HIC_%s_%d" % t for t in zip(n1, rng.randint(1, 900000, n).tolist())),
               ("HIC_%s_%d" % t for t in zip(n2, rng.randint(1, 900000, n).tolist())),
               map(str, rng.randint(0, 61, n).tolist()), map(str, rng.randint(0, 61, n).tolist()))
    return ("\n".join(map("\t".join, rows)) + "\n").encode()


def chrom_features(n: int, d: int, n_labels: int, seed: int, positive_rate: float = 0.05) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    return {"forward": torch.randn(n, d, generator=g), "backward": torch.randn(n, d, generator=g),
            "target": (torch.rand(n, n_labels, generator=g) < positive_rate).float()}


def synthetic_chromosome(chrom: str, d: int = 128, n_labels: int = N_LABELS, pairs: int = PAIRS_PER_CHROM,
                         hic_like: bool = False, n: int = None) -> Tuple[Dict[str, torch.Tensor], sp.csr_matrix]:
    n = chrom_nodes(chrom) if n is None else n
    seed = chrom_seed(chrom)
    return chrom_features(n, d, n_labels, 1000 + seed), contact_graph(n, pairs, seed, hic_like)


def config1(d: int = 128, n_labels: int = N_LABELS):
    """BASELINE.json configs[0]: one chromosome, 5k nodes, ~1 % density."""
    n = 5000
    return chrom_features(n, d, n_labels, 1000), contact_graph(n, int(0.01 * n * n / 2), 0)
