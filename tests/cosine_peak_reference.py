"""The yardstick of the peak-search tests (``naf.locate``, ``ops.xna_cos_peaks``, ``ops.peaks_topk``; naf_xna_cos_peaks_fwd, naf_peaks_topk).

1. The definition.  With ``cos`` [B, N, Ho, Wo] the scaled cosines (tests/cosine_reference.py) and an integer ratio dy = Ho / h, dx = Wo / w,
   cell (cy, cx) = the pixels [cy*dy, (cy+1)*dy) x [cx*dx, (cx+1)*dx):
       peak[b, n, cy, cx]  = max of cos[b, n] over the cell
       where[b, n, cy, cx] = the lowest flat index y * Wo + x among the cell's pixels that attain it
   ``cell_peaks`` states it with torch reductions, ``cell_peaks_loop`` pixel by pixel (tests/test_cosine_peaks_cpu.py holds one to the other).
   Top-k: the h * w candidates (peak, where) of a (b, n) ordered by value descending, then by flat index ascending; the first k
   (``topk_reference``, ``topk_loop``).

2. Against fp64.  The maximum is 1-Lipschitz in the sup norm: with |cos~ - ref| <= bound per element (cosine_reference.bound),
       |peak - max_cell ref| <= max_cell bound,
   and the reported pixel p has ref[p] >= cos~[p] - bound[p] = peak - bound[p] >= max_cell ref - 2 max_cell bound.  Nothing is measured.

3. ``emulate``: the kernel's merge order on the host (naf_amd/csrc/xna_cos_kernel.h, peak epilogue) -- row tiles of 16 lanes, lanes past a
   partial last tile repeating the row's last pixel, tiles dealt to eight waves in rounds of 8 * tiles-per-wave, per-wave running pairs,
   the merge of the waves -- with one planted defect per keyword; tests/test_cosine_peaks_cpu.py states the input on which each changes
   the result.

A helper (no tests in it).
"""
import torch

INT_MAX = 2 ** 31 - 1
NW = 8            # waves of a workgroup


def cell_peaks(cos, h, w):
    """(peak [B, N, h, w] of cos's dtype, where [B, N, h, w] int32) by torch reductions."""
    B, N, Ho, Wo = cos.shape
    assert Ho % h == 0 and Wo % w == 0
    dy, dx = Ho // h, Wo // w
    c = cos.reshape(B, N, h, dy, w, dx)
    peak = c.amax(dim=(3, 5))
    idx = torch.arange(Ho * Wo, dtype=torch.int64, device=cos.device).view(1, 1, h, dy, w, dx)
    where = torch.where(c == peak[:, :, :, None, :, None], idx, torch.full_like(idx, INT_MAX)).amin(dim=(3, 5))
    return peak, where.to(torch.int32)


def cell_peaks_loop(cos, h, w):
    """The same, pixel by pixel in flat-index order: a later pixel replaces the running maximum only when strictly greater."""
    B, N, Ho, Wo = cos.shape
    dy, dx = Ho // h, Wo // w
    peak = torch.empty(B, N, h, w, dtype=cos.dtype)
    where = torch.empty(B, N, h, w, dtype=torch.int32)
    for b in range(B):
        for n in range(N):
            for cy in range(h):
                for cx in range(w):
                    best, at = None, -1
                    for y in range(cy * dy, (cy + 1) * dy):
                        for x in range(cx * dx, (cx + 1) * dx):
                            v = float(cos[b, n, y, x])
                            if best is None or v > best:
                                best, at = v, y * Wo + x
                    peak[b, n, cy, cx], where[b, n, cy, cx] = best, at
    return peak, where


def topk_reference(peak, where, k):
    """(values [B, N, k], index [B, N, k] int32): two stable sorts, by index ascending and then by value descending."""
    B, N = peak.shape[:2]
    p, i = peak.reshape(B, N, -1), where.reshape(B, N, -1).long()
    o1 = torch.sort(i, dim=2, stable=True).indices
    p1, i1 = p.gather(2, o1), i.gather(2, o1)
    o2 = torch.sort(p1, dim=2, descending=True, stable=True).indices
    return p1.gather(2, o2)[:, :, :k].contiguous(), i1.gather(2, o2)[:, :, :k].to(torch.int32).contiguous()


def topk_loop(peak, where, k):
    """The same by Python's sort on (-value, index)."""
    B, N = peak.shape[:2]
    vals, idx = torch.empty(B, N, k, dtype=peak.dtype), torch.empty(B, N, k, dtype=torch.int32)
    for b in range(B):
        for n in range(N):
            c = sorted(zip(peak[b, n].reshape(-1).tolist(), where[b, n].reshape(-1).tolist()), key=lambda t: (-t[0], t[1]))[:k]
            vals[b, n] = torch.tensor([t[0] for t in c], dtype=peak.dtype)
            idx[b, n] = torch.tensor([t[1] for t in c], dtype=torch.int32)
    return vals, idx


def check_against_fp64(peak, where, ref, bnd, h, w, what):
    """2 of the module docstring, every cell, NaN counts as a miss."""
    B, N, Ho, Wo = ref.shape
    dy, dx = Ho // h, Wo // w
    rmax = ref.reshape(B, N, h, dy, w, dx).amax(dim=(3, 5))
    bmax = bnd.reshape(B, N, h, dy, w, dx).amax(dim=(3, 5))
    err = (peak.double() - rmax).abs()
    print(f"{what}: max |peak - max ref| {float(err.max()):.3e}, worst / bound {float((err / bmax.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bmax).all()), f"{what}: {int((~(err <= bmax)).sum())} cell maxima outside the bound"
    wl = where.long()
    cy, cx = (wl // Wo) // dy, (wl % Wo) // dx
    gy = torch.arange(h).view(1, 1, h, 1).expand_as(wl)
    gx = torch.arange(w).view(1, 1, 1, w).expand_as(wl)
    assert bool(((cy == gy) & (cx == gx)).all()), f"{what}: an index outside its cell"
    at = ref.reshape(B, N, Ho * Wo).gather(2, wl.reshape(B, N, h * w)).view(B, N, h, w)
    short = rmax - at
    print(f"{what}: worst (max ref - ref[where]) / (2 bound) {float((short / (2 * bmax).clamp_min(1e-300)).max()):.3f}")
    assert bool((at >= rmax - 2 * bmax).all()), f"{what}: {int((~(at >= rmax - 2 * bmax)).sum())} locations worse than 2 bounds below the maximum"


DEFECTS = ("tie_high", "ghost_lane", "dead_tile", "round_replace", "drop_wave", "cell_coords", "swap_yx", "max_before_scale")


def emulate(c, ls, h, w, tpw=2, defect=None):
    """The kernel's merge on the host for UNSCALED cosines ``c`` [Ho, Wo] fp32 of one (b, n) and the scale ``ls``: (peak [h, w] fp32,
    where [h, w] int32).  z = fp32(ls * c) per pixel, as the epilogue forms it.  Defects (one keyword):
      tie_high          equal values keep the HIGHER index (in the tile, in the wave's slot and in the merge)
      ghost_lane        a lane past a partial last tile reads the pixel at its own x (the neighbouring cell's) and counts it at that index
      dead_tile         a tile past the cell takes part, with the rows below the cell it would address
      round_replace     a wave's result of a later round replaces its earlier one
      drop_wave         the last wave is left out of the merge
      cell_coords       the index is y * dx + x in the cell's own coordinates
      swap_yx           the index is x * Wo + y
      max_before_scale  the maximum is taken over c and scaled afterwards"""
    assert defect is None or defect in DEFECTS
    Ho, Wo = c.shape
    dy, dx = Ho // h, Wo // w
    c = c.float()
    ls32 = torch.tensor(ls, dtype=torch.float32)
    z = (c if defect == "max_before_scale" else ls32 * c).tolist()
    tpr = (dx + 15) // 16
    ntile = dy * tpr
    peak = torch.empty(h, w, dtype=torch.float32)
    where = torch.empty(h, w, dtype=torch.int32)

    def before(av, ai, bv, bi):
        return av > bv or (av == bv and (ai > bi if defect == "tie_high" else ai < bi))

    for cy in range(h):
        for cx in range(w):
            slots = [(float("-inf"), INT_MAX if defect != "tie_high" else -1) for _ in range(NW)]
            for rnd, t0 in enumerate(range(0, ntile, NW * tpw)):
                fresh = [True] * NW
                for u in range(tpw):
                    for wave in range(NW):
                        tt = t0 + u * NW + wave
                        if tt >= ntile and defect != "dead_tile":
                            continue
                        ttc = tt if defect == "dead_tile" else min(tt, ntile - 1)
                        ty, tx0 = ttc // tpr, (ttc % tpr) * 16
                        gy = min(cy * dy + ty, Ho - 1)
                        best = None
                        for col in range(16):
                            xl = tx0 + col
                            if xl >= dx:
                                if defect != "ghost_lane":
                                    xl = dx - 1          # the row's last pixel again, at its own index
                                elif cx * dx + xl >= Wo:
                                    continue
                            gx = cx * dx + xl
                            if defect == "cell_coords":
                                i = ty * dx + xl
                            elif defect == "swap_yx":
                                i = gx * Wo + gy
                            else:
                                i = gy * Wo + gx
                            cand = (z[gy][gx], i)
                            if best is None or before(*cand, *best):
                                best = cand
                        if defect == "round_replace" and rnd > 0 and fresh[wave]:
                            slots[wave] = best
                        elif before(*best, *slots[wave]):
                            slots[wave] = best
                        fresh[wave] = False
            best = slots[0]
            for wave in range(1, NW - 1 if defect == "drop_wave" else NW):
                if before(*slots[wave], *best):
                    best = slots[wave]
            v = best[0]
            if defect == "max_before_scale":
                v = float(ls32 * torch.tensor(v, dtype=torch.float32))
            peak[cy, cx], where[cy, cx] = v, best[1]
    return peak, where
