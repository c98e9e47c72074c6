"""The inputs of the class-embedding maps of scripts/visualize.py:148-188: the GCN's hidden representation of the windows
that carry exactly one label, for the labels with enough such windows, both strands averaged (:152).

The reference collects `all_single_class_z` / `all_single_class_targs` in code it does not ship; the hidden state is defined
here as ChromeGCN.hidden_strands (the output of the gated stack, the classifier's input).  Everything stays on the device;
chromegcn_amd.tsne embeds the result."""
from __future__ import annotations

from typing import Iterable, Optional

import numpy as np
import torch

from . import ops


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _selection(single_label: torch.Tensor, is_single: torch.Tensor, C: int, labels: Optional[Iterable[int]], min_count: int):
    """rows (int64, window order within ascending label order) and their labels, from every window's label and whether it
    is its only one"""
    counts = torch.bincount(single_label[is_single], minlength=C)
    keep = counts >= int(min_count)
    if labels is not None:
        wanted = torch.zeros(C, dtype=torch.bool, device=keep.device)
        idx = torch.as_tensor([int(c) for c in labels], dtype=torch.int64, device=keep.device)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= C):
            raise ValueError("class_embeddings: a label outside [0, %d)" % C)
        wanted[idx] = True
        keep &= wanted
    rows = torch.nonzero(is_single & keep[single_label]).view(-1)
    order = torch.sort(single_label[rows], stable=True).indices    # stable: window order inside a label
    rows = rows[order]
    return rows, single_label[rows]


def class_embeddings(model, x_f, x_r, adj, targets, labels=None, min_count: int = 200):
    """(z [m, d] float32, label [m] int64, rows [m] int64), all on the device.
    model: chromegcn_amd.ChromeGCN; x_f, x_r: [n, d] features of the forward and the reverse-complement strand; adj: what
    as_graph accepts; targets: [n, C], nonzero = positive.  Each of the four may also be a list with one entry per
    chromosome; the chromosomes are concatenated in the order given and `rows` indexes the concatenation.
    A window is kept when its target row has exactly one positive (`label`), that label is in `labels` (default: all) and
    at least `min_count` kept windows carry it (the reference's `len(i_nonzero) > 199`, visualize.py:164).  z is the mean
    of the two strands' hidden rows (:152, ChromeGCN.hidden_strands).  Order: ascending label, window order inside a label,
    as the reference's loop over labels concatenates them (:162-170)."""
    xs_f, xs_r, adjs, tgs = _as_list(x_f), _as_list(x_r), _as_list(adj), _as_list(targets)
    if not (len(xs_f) == len(xs_r) == len(adjs) == len(tgs)):
        raise ValueError("class_embeddings: x_f, x_r, adj and targets must list the same chromosomes (%d, %d, %d, %d)"
                         % (len(xs_f), len(xs_r), len(adjs), len(tgs)))
    hidden, tg_all = [], []
    for xf, xr, a, tg in zip(xs_f, xs_r, adjs, tgs):
        ops._require_cuda(xf, "x_f")
        ops._require_cuda(xr, "x_r")
        if tuple(tg.shape[:1]) != (xf.shape[0],) or tg.dim() != 2:
            raise ValueError("class_embeddings: targets must be [n, C] with n = %d, got %s" % (xf.shape[0], tuple(tg.shape)))
        h = model.hidden_strands(torch.stack([xf.detach(), xr.detach()]), a)
        hidden.append((h[0] + h[1]) / 2)
        tg_all.append(tg.to(xf.device) != 0)
    with torch.no_grad():
        z_all, pos = torch.cat(hidden), torch.cat(tg_all)
        rows, label = _selection(pos.to(torch.int32).argmax(1), pos.sum(1) == 1, pos.shape[1], labels, min_count)
        return z_all[rows], label, rows


def select_single_label_host(targets, labels=None, min_count: int = 200):
    """The same selection in numpy, as the reference's loop states it: (rows, label) for targets [n, C] (one array, or a
    list of them, concatenated)."""
    t = np.concatenate([np.asarray(a) != 0 for a in _as_list(targets)])
    single = np.flatnonzero(t.sum(1) == 1)
    lab = t[single].argmax(1)
    rows, out = [], []
    for c in (range(t.shape[1]) if labels is None else sorted(set(int(c) for c in labels))):
        hit = single[lab == c]
        if len(hit) > int(min_count) - 1:
            rows.append(hit)
            out.append(np.full(len(hit), c, np.int64))
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(rows).astype(np.int64), np.concatenate(out)
