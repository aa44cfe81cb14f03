"""TEST INFRASTRUCTURE: the per-slice error statistic of the kernel parity checks.

A whole-tensor relative L2 norm averages a localised error away: one wrong channel of 384, one halo row, one 16-row tile, one
sample with another sample's DropPath factor all stay far below the 16-bit tolerances.  `slice_err` looks at every axis of the
reference and every index on it:

    e(axis, i) = rms(got - ref over the slice) / max(rms(ref over the slice), rms(ref over the whole tensor))

and returns the largest with its place.  The global rms in the denominator keeps slices whose reference is legitimately ~0 (a sample
whose DropPath keep is 0, padded channels) from raising alarms; a slice of fewer than MIN_SLICE elements is joined with its
neighbours on that axis into blocks of at least MIN_SLICE (1-D tensors, the 9-tap axis of a (9, C) tap gradient).  With
geom = (B, H, W) an (M, C) token tensor is looked at as (B, H, W, C): samples, image rows and image columns are axes of their own, and
the M token rows stay slices as well.  A window-major tensor (one row per 8x8 window) keeps its rows.  Everything is computed in
fp64 on the CPU."""
import collections

import torch

MIN_SLICE = 16

Worst = collections.namedtuple("Worst", "err axis index stop name")          # slice [index, stop) of `axis`; name: "channel", "image row", ...


def where(w):
    """'channel 383' / 'row [16:32)'"""
    return "%s %d" % (w.name, w.index) if w.stop == w.index + 1 else "%s [%d:%d)" % (w.name, w.index, w.stop)


def _names(ndim, geom_applied):
    if geom_applied:
        return (["sample", "image row", "image column"] + ["axis %d" % a for a in range(3, ndim - 1)] + ["channel"])[:ndim]
    if ndim == 1:
        return ["element"]
    if ndim == 2:
        return ["row", "channel"]
    return ["axis %d" % a for a in range(ndim - 1)] + ["channel"]


def view_geom(t, geom):
    """an (M, ...) token tensor with M == B H W as (B, H, W, ...); a tensor that already starts (B, H, W) stays; anything else (a
    window-major gate, a parameter gradient handled by the same check) is not token-major and keeps its own axes"""
    if geom is None:
        return t, False
    B, H, W = (int(v) for v in geom)
    if t.dim() >= 3 and tuple(t.shape[:3]) == (B, H, W):
        return t, True
    if t.dim() >= 1 and t.shape[0] == B * H * W and B * H * W > 1:
        return t.reshape((B, H, W) + tuple(t.shape[1:])), True
    return t, False


def _blocks(n, per):
    """[start, stop) of the groups of consecutive indices on an axis of n slices with `per` elements each: groups of
    ceil(MIN_SLICE / per), a short tail joined to the group before it"""
    g = max(1, -(-MIN_SLICE // max(per, 1)))
    starts = list(range(0, n, g))
    if len(starts) > 1 and n - starts[-1] < g:
        starts.pop()
    return starts, starts[1:] + [n]


def slice_err(got, ref, geom=None):
    """Worst(err, axis, index, stop, name): the largest e(axis, i) over every axis of `ref` (after the geom view).  A non-finite
    element of `got` where `ref` is finite gives err = inf at its place; a NaN anywhere else in the statistic gives err = NaN (which
    fails every `<`)."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    ref = torch.as_tensor(ref).detach().cpu().to(torch.float64)
    assert got.numel() == ref.numel(), (tuple(got.shape), tuple(ref.shape))
    if ref.dim() == 0:
        got, ref = got.reshape(1), ref.reshape(1)
    ref, applied = view_geom(ref, geom)
    got = got.reshape(ref.shape)
    names = _names(ref.dim(), applied)
    bad = None if bool(torch.isfinite(got).all()) else ~torch.isfinite(got) & torch.isfinite(ref)
    if bad is not None and bool(bad.any()):
        idx = [int(v) for v in bad.nonzero()[0]]
        axis = len(idx) - 1
        return Worst(float("inf"), axis, idx[axis], idx[axis] + 1, "non-finite at index %s: %s" % (tuple(idx), names[axis]))
    d2, r2 = (got - ref).square_(), ref * ref
    n_all = ref.numel()
    g_ms = float(r2.sum()) / max(n_all, 1)
    worst, top = Worst(0.0, 0, 0, 1, names[0]), 0.0
    if n_all == 0:
        return worst
    # the last axis straight from the full tensors, the others from the (small) sums over it
    last = ref.dim() - 1
    lead = tuple(range(last))
    per_axis = [None] * ref.dim()
    per_axis[last] = (d2.sum(dim=lead), r2.sum(dim=lead)) if lead else (d2, r2)
    if lead:
        d2l, r2l = d2.sum(dim=last), r2.sum(dim=last)
        for a in lead:
            others = tuple(x for x in lead if x != a)
            per_axis[a] = (d2l.sum(dim=others), r2l.sum(dim=others)) if others else (d2l, r2l)
    axes = [(a, names[a], ref.shape[a], sd, sr) for a, (sd, sr) in enumerate(per_axis)]
    if applied and ref.dim() == 4:
        # the token rows stay slices of their own next to the image axes: one wrong pixel, one wrong 16-row tile
        axes.append((4, "token", d2l.numel(), d2l.flatten(), r2l.flatten()))
    for a, name, n, sd, sr in axes:
        per = n_all // n
        starts, stops = _blocks(n, per)
        if len(starts) < n:
            cd, cr = torch.cat([sd.new_zeros(1), sd.cumsum(0)]), torch.cat([sr.new_zeros(1), sr.cumsum(0)])
            s, e = torch.tensor(starts), torch.tensor(stops)
            sd, sr = cd[e] - cd[s], cr[e] - cr[s]
            cnt = (e - s).to(torch.float64) * per
        else:
            cnt = torch.full((n,), float(per), dtype=torch.float64)
        den = torch.maximum(sr / cnt, torch.full_like(sr, g_ms)).sqrt().clamp_min(1e-30)
        e_ = (sd.clamp_min(0) / cnt).sqrt() / den
        if bool(torch.isnan(e_).any()):
            k = int(torch.isnan(e_).nonzero()[0])
            return Worst(float("nan"), a, starts[k], stops[k], name)
        k = int(e_.argmax())
        top = max(top, float(e_[k]))
        # the place: an axis named earlier (the image axes before the channels before the single tokens) keeps it unless a later one is
        # clearly worse -- every token of a wrong sample is as wrong as the sample
        if float(e_[k]) > 1.05 * worst.err:
            worst = Worst(float(e_[k]), a, starts[k], stops[k], name)
    return worst._replace(err=top)
