#!/usr/bin/env python
"""Generate naf_amd/csrc/stem_rows_sched.inc: the hand-placed instruction schedule of the row-streaming 3x3 stem layer
(stem_conv_rows_kernel, stem_rows_kernel.h), as straight-line HIP.

    python tools/gen_stem_rows.py [out.inc]      # rewrites the .inc (committed; the build does not run this)

One wave per SIMD issues in order, so side work hides only in the 16-cycle shadow of individual MFMAs
(v_mfma_f32_16x16x32_bf16): every micro-op is pinned behind the MFMA of its slot (sched_barrier + asm register anchors).

The body is two double-steps (D = 0, 1) of 288 MFMA slots = 2 input rows x 24 fragments x 3 output rows x 2 channel tiles.
Input row t (t = 2 D + tt, names mod 4) feeds output row (t-1)&3 with tap row 2 (that output row is finished by it), t&3 with
tap row 1 and (t+1)&3 with tap row 0 (that row starts here, from the conv bias); output row (t+2)&3 -- image row t-2 -- has its
epilogue during row t and is then re-initialised with the bias straight from the LDS.  Side work of a double-step: the scalar
row pointers / masks (u_all, slot 0), GroupNorm + SiLU + ring write of the five 16-byte pieces of batch d+2 (plain f32 VALU
only), their reload with batch d+3 right after they are unpacked, the four row-store pieces of the previous tile (tile read
twelve slots ahead of its store), eight epilogue slices of six micro-ops each.

Placement budget: the MFMA holds the SIMD's vector issue for 8 of its 16 cycles, a plain VALU instruction costs 4 and a
transcendental 8 -- so a slot takes two plain instructions, or one transcendental ALONE, and every micro-op is cut to that
size.  The side work sums to about 0.9 of the budget of a double-step: there is no slack to front-load anything, the
greedy placement (earliest slot with room, dependency gaps below) just fills the slots in order.  A micro-op dearer than
a whole slot (a global load or store with its address, the scalar block) gets a slot with nothing else in it and
lengthens that one gap.  The MFMA macro of the kernel puts a sched_barrier behind every MFMA and NAF_SLOT_PIN one behind
every slot, so what is placed here is what issues there.
"""
import os
import sys

NB = 3                      # B-fragment buffers: a fragment is requested 3 fragments = 18 MFMAs ahead
NLD, NST = 5, 4
NSLOT = 288
FR = 6                      # MFMAs per fragment: 3 output rows x 2 channel tiles
ROW = 24 * FR               # slots per input row
# Placement budget per MFMA gap: 16 cycles, 8 of them the MFMA's own hold on the SIMD's vector issue, so CAP = 8 cycles of
# VALU issue (plain 4, transcendental 8) and beside them OTH instructions that issue elsewhere (LDS, scalar, vector memory).
CAP = float(os.environ.get("NAF_ROWS_CAP", "8"))
OTH = int(os.environ.get("NAF_ROWS_OTH", "1"))
V, TR = 4.0, 8.0


class Budget:
    """Per-slot load of one instantiation: VALU issue cycles and the count of other instructions."""

    def __init__(self, valu, oth, cap, ocap, what):
        self.valu, self.oth, self.cap, self.ocap, self.what = list(valu), list(oth), cap, ocap, what

    def place(self, v, o, earliest):
        # earliest slot with room; a micro-op dearer than a whole slot takes one that holds nothing yet and lengthens that gap
        k = max(0, earliest)
        while k < NSLOT - 1 and not ((self.valu[k] + v <= self.cap and self.oth[k] + o <= self.ocap) or (self.valu[k] == 0 and self.oth[k] == 0)):
            k += 1
        assert k < NSLOT - 1, self.what + " does not fit"
        self.valu[k] += v
        self.oth[k] += o
        return k


def build(D):
    bud = Budget([0.0] * NSLOT, [0] * NSLOT, CAP, OTH, "schedule")
    ops = [[] for _ in range(NSLOT)]        # (kind, code) behind the MFMA of the slot
    pre = [[] for _ in range(NSLOT)]        # before the MFMA of the slot

    # fragment requests: behind the last use of every fragment
    for k in range(NSLOT):
        if k % FR == FR - 1:
            bud.oth[k] += 1
    place = bud.place

    # ---- the double-step's uniform row pointers and masks: first thing behind the first MFMA ----
    bud.oth[0] += 10
    ops[0].append(("uni", "u_all();"))

    # ---- epilogues: output row tt of the tile = output row name (2 D + tt + 2) & 3, during input row tt ----
    EPI = [(2 * V, 0), (V, 1), (2 * V, 0), (2 * V, 0), (2 * V, 0), (2 * V, 0)]     # cvt x 2 | tile write, add | add x 2 | mul, fma | fma x 2 | mask, fma x 2
    for tt in range(2):
        nm = (2 * D + tt + 2) & 3
        k = ROW * tt + 7           # its last MFMA was slot ROW - 5 of the row before: 12 slots = 192 cycles behind it
        for j in range(4):
            for part in range(6):
                k = place(*EPI[part], k + 1)
                ops[k].append(("epi", f"epi{part}({nm}, {tt}, {j});"))
        # bias back into the accumulators: they are tap row 0 of the next input row
        for j in range(4):
            k = place(0, 1, k + 1)
            ops[k].append(("epi", f"acc_init({nm}, {j});"))
        assert k < ROW * (tt + 1) - 8, "accumulator re-initialisation too late"

    # ---- row stores of the previous tile ----
    k = 80
    for n in range(NST):
        k = place(0, 1, k + 1)
        pre[k].append(("store", f"stv = *reinterpret_cast<const u32x4_t*>(prev_tile + st_lds0 + {16 * n} * PXE);"))
        k2 = place(V, 1, k + 12)    # the tile read has to come back first: LDS latency, in order behind the fragment reads
        ops[k2].append(("store", f"if (!EDGE || st_ok({n})) {{ uint32_t o_ = st_goff0; NAF_PIN1(o_); *reinterpret_cast<u32x4_t*>(prev_row{n // 2} + {'st_px16 + ' if n % 2 else ''}o_) = stv; }}"))
        k = k2

    # ---- commits (one variable set: piece n+1 starts after piece n has stored) ----
    start = 1
    for n in range(NLD):
        start = max(start, 1 + 54 * n)      # spread the pieces over the double-step
        t = {}
        def put(name, cost, earliest, code, kind="commit", oth=0):
            k = place(cost, oth, earliest)
            ops[k].append((kind, code))
            t[name] = k
            return k
        # Plain (non-packed) f32 VALU only: a v_pk_*_f32 beside an MFMA stalls the matrix pipe, a plain v_fma does not
        # (profiles/r03_mfma_filler_prices.txt).  ys = log2(e) * GroupNorm(x) (the scale is folded into gav / gbv), so
        # SiLU(y) = ys * rcp(log2e + log2e * exp2(-ys)): the exp2's negation is an input modifier, the "1 +" an fma.
        for p in range(4):
            a_earliest = start if p == 0 else t[f"A{p - 1}"]
            put(f"A{p}", 2 * V, a_earliest,
                f"{{ const uint32_t w_ = ld[{n}][{p}]; cy[{2 * p}] = __uint_as_float(w_ << 16); cy[{2 * p + 1}] = __uint_as_float(w_ & 0xffff0000u); "
                f"NAF_PIN2(cy[{2 * p}], cy[{2 * p + 1}]); }}")
        # the piece's registers are free again: reload them with the same piece of batch d + 3
        r_lo, r_hi = (16 * n) // 40, (16 * n + 15) // 40
        ops[t["A0"]].append(("copy", f"NAF_LDS_WRITE_2X64(commit_base + c_off({n}), ld[{n}][0], ld[{n}][1], ld[{n}][2], ld[{n}][3]);"))
        if r_lo == r_hi:
            put("L", V, t["A3"],
                f"{{ uint32_t o_ = col_off[{n}]; NAF_PIN1(o_); NAF_LD_DST({n}) = *reinterpret_cast<const u32x4_t*>(next_row{r_lo} + o_); }}", kind="load", oth=1)
        else:   # the piece that straddles the batch's two rows: one base (the lower row), the row stride in the lane's offset
            put("L", 2 * V, t["A3"],
                f"{{ uint32_t o_ = (straddle_hi != next_flip) ? col_off_s1 : col_off[{n}]; NAF_PIN1(o_); "
                f"NAF_LD_DST({n}) = *reinterpret_cast<const u32x4_t*>(next_lo + o_); }}", kind="load", oth=1)
        for p in range(4):
            a, b = 2 * p, 2 * p + 1
            put(f"B{p}", 2 * V, t[f"A{p}"] + 1,
                f"{{ cy[{a}] = __builtin_fmaf(cy[{a}], gav[{a}], gbv[{a}]); cy[{b}] = __builtin_fmaf(cy[{b}], gav[{b}], gbv[{b}]); NAF_PIN2(cy[{a}], cy[{b}]); }}")
            for q, e in enumerate((a, b)):     # a transcendental fills its slot alone
                put(f"C{p}{q}", TR, t[f"B{p}"] + 1, f"{{ cu[{e}] = __builtin_amdgcn_exp2f(-cy[{e}]); NAF_PIN1(cu[{e}]); }}")
            put(f"D{p}", 2 * V, max(t[f"C{p}0"], t[f"C{p}1"]) + 2,
                f"{{ cu[{a}] = __builtin_fmaf(cu[{a}], kL, kL); cu[{b}] = __builtin_fmaf(cu[{b}], kL, kL); NAF_PIN2(cu[{a}], cu[{b}]); }}")
            for q, e in enumerate((a, b)):
                put(f"E{p}{q}", TR, t[f"D{p}"] + 1, f"{{ cu[{e}] = __builtin_amdgcn_rcpf(cu[{e}]); NAF_PIN1(cu[{e}]); }}")
            put(f"F{p}", 2 * V, max(t[f"E{p}0"], t[f"E{p}1"]) + 2,
                f"{{ cy[{a}] = cy[{a}] * cu[{a}]; cy[{b}] = cy[{b}] * cu[{b}]; NAF_PIN2(cy[{a}], cy[{b}]); }}")
            put(f"H{p}", V, t[f"F{p}"] + 1,
                f"{{ bf16x2_t o_; o_[0] = (bf16_t)cy[{a}]; o_[1] = (bf16_t)cy[{b}]; co[{p}] = __builtin_bit_cast(uint32_t, o_); NAF_PIN1(co[{p}]); }}")
        g = 0
        for h in range(2):      # 16 bytes into the ring as two ds_write_b64, one per slot
            g = put(f"G{h}", V, max(t[f"H{2 * h}"], t[f"H{2 * h + 1}"], g) + 1,
                    f"NAF_LDS_WRITE_64(commit_base + c_off({n}) + {4 * h}, co[{2 * h}], co[{2 * h + 1}]);", oth=1)
        start = g + 1
    last_commit = start

    # ---- POOL instantiation (naf_stem_conv_keys_fwd): the previous double-step's tile -> the cells' sums, see stem_rows_kernel.h ----
    # Per tile row g: the row's indicator operand, then four chains (fragment read -> small MFMA six slots later -> its result
    # joins the sums in the LDS four slots behind it; an asm MFMA has no hazard recogniser between it and its consumers: the
    # distances are those of the 32-cycle schedule in cycles, twice as many slots).  In D = 0 the finished band's keys sit between
    # the two rows, under `if (pfin)` (one double-step in eight).  Everything is placed on top of the schedule above with a
    # slightly larger budget (the small MFMAs are not side work: they follow their slot's MFMA, and the POOL instantiation has
    # no GroupNorm sums in its epilogue slices); `if constexpr (POOL)` removes all of it elsewhere.
    PDIST = int(os.environ.get("NAF_ROWS_POOL_DIST", "6"))     # slots between a chain's LDS reads and its MFMA
    pool = [[] for _ in range(NSLOT)]
    lp = list(bud.valu)
    for k in range(NSLOT):          # the epilogue slices' sums do not exist in this instantiation
        for kind, code in ops[k]:
            if kind == "epi" and code.startswith("epi") and code[3] in "2345":
                lp[k] -= 2 * V
            elif code.startswith("epi1"):
                lp[k] -= V
    pbud = Budget(lp, bud.oth, CAP + float(os.environ.get("NAF_ROWS_POOL_EXTRA", "4")), OTH + 1, "pool schedule")
    def pl(v, o, earliest):
        return pbud.place(v, o, earliest)
    # the keys' own budget (D = 0 only): one double-step in eight may run over
    kbud = Budget(lp, bud.oth, CAP + float(os.environ.get("NAF_ROWS_POOL_BND_EXTRA", "20")), OTH + 6, "pool keys")
    def plb(v, o, earliest):
        return kbud.place(v, o, earliest)
    k = 6                   # chain cursor: one accumulator register set, so the chains follow each other
    for g in range(2):
        ka = pl(2 * V, 1, k)
        pool[ka].append(("", f"pool_a0(pr0 + {g});"))
        ka = pl(2 * V, 0, ka + 4)
        pool[ka].append(("", "pool_a1();"))
        k = max(k, ka)
        for q in range(4):
            kr = pl(0, 2, k)    # sums so far + tile fragment
            pool[kr].append(("", f"pool_rd(prev_tile, {g}, {q});"))
            km = pl(8.0, 0, max(kr + PDIST, ka + 2))
            pool[km].append(("", "pool_mm();"))
            ks = pl(0, 2, km + 4)
            pool[ks].append(("", f"pool_st({q}, 0); pool_st({q}, 1);"))
            k = ks
        if g == 0 and D == 0:       # the band's keys between the two rows' chains (not beside them: the chains' registers are free then)
            kf = k + 1
            for c in range(2):
                for i in range(4):
                    kf = plb(0, 6, kf)
                    pool[kf].append(("pfin", f"pool_f0(pr0, {c}, {i});"))
                    kf = plb(4 * V, 0, kf + 6)
                    pool[kf].append(("pfin", f"pool_f1({i});"))
                    kf += 1
                for w in range(2):
                    kf = plb(4 * V, 0, kf)
                    pool[kf].append(("pfin", f"pool_f2({w});"))
                    kf += 1
                kf = plb(4 * V, 1, kf)
                pool[kf].append(("pfin", f"pool_f3(pr0, {c});"))
                kf += 1
            k = kf
    pool_done = k

    # ---- emit ----
    out = []
    for k in range(NSLOT):
        tt, r = divmod(k, ROW)
        f, w6 = divmod(r, FR)
        u, a = divmod(w6, 2)
        t_row = 2 * D + tt
        nm = [(t_row - 1) & 3, t_row & 3, (t_row + 1) & 3][u]
        dy = 2 - u
        dx, b, ks = f >> 3, (f >> 2) & 1, f & 3
        fi = tt * 24 + f
        widx = ((dy * 3 + dx) * 2 + a) * 4 + ks
        if w6 == 0 and f == 0:
            out.append(f"// ---- input row {t_row} of the body: finishes output row {(t_row - 1) & 3}, starts {(t_row + 1) & 3}; epilogue of {(t_row + 2) & 3}")
        if pre[k]:
            out.append("__builtin_amdgcn_sched_barrier(0);")
            for kind, code in pre[k]:
                out.append(f"if constexpr (!(ABL & 8)) {{ {code} }}")
            out.append("__builtin_amdgcn_sched_barrier(0);")
        # explicit register classes: accumulators and B fragments in VGPRs, weights in AGPRs except the 8 fragments of tap
        # (0, 0) (288 weight registers > 256 AGPRs).  An asm MFMA is invisible to hipcc's hazard recogniser; the schedule keeps
        # every accumulator's first VALU read >= 12 MFMA slots behind its last MFMA, B fragments come from ds_read (waitcnt is
        # still tracked per register) and nothing but MFMAs writes the accumulators between acc_init and the epilogue.
        wcls = "v" if widx < 8 else "a"
        out.append(f"NAF_MFMA(acc[{nm}][{2 * a + b}], wreg[{widx}], bb[{fi % NB}], \"{wcls}\");  // slot {k}")
        if w6 == FR - 1:
            nf = fi + NB
            if nf < 24:
                base = f"cur + {2 * D} * ROWE"
            elif nf < 48:
                base = f"cur + {2 * D + 1} * ROWE"
            else:
                base = "cur + 2 * ROWE" if D == 0 else "oth"
            out.append(f"load_frag({base}, {nf % 24}, bb[{fi % NB}]);")
        for kind, code in ops[k]:
            if kind == "store":
                out.append(f"if constexpr (!(ABL & 8)) {{ {code} }}")
            elif kind in ("epi", "uni"):
                out.append(code)
            elif kind == "load":
                out.append(f"if constexpr (!(ABL & 16)) {{ {code} }}")
            elif kind == "copy":
                out.append(f"if constexpr (PLAIN && !(ABL & 1)) {{ {code} }}")
            else:
                out.append(f"if constexpr (!PLAIN && !(ABL & 1)) {{ {code} }}")
        for cond, code in pool[k]:
            if cond:
                out.append(f"if constexpr (POOL) {{ if ({cond}) {{ {code} }} }}")
            else:
                out.append(f"if constexpr (POOL) {{ {code} }}")
        out.append("NAF_SLOT_PIN;")
    load = bud.valu
    over = sum(max(0.0, x - CAP) for x in load)
    return out, load, last_commit, over, pool_done


text = ["// GENERATED by tools/gen_stem_rows.py -- do not edit.  One double-step (two input rows, 288 MFMA slots) of",
        "// stem_conv_rows_kernel per value of NAF_ROWS_D, side work pinned behind individual MFMAs."]
stats = []
for D in (0, 1):
    body, load, last_commit, over, pool_done = build(D)
    text.append(f"#if NAF_ROWS_D == {D}")
    text += body
    text.append("#endif")
    stats.append((max(load), sum(load), last_commit, over, pool_done))

path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "naf_amd", "csrc", "stem_rows_sched.inc")
if len(sys.argv) > 1:
    path = sys.argv[1]
with open(path, "w") as fh:
    fh.write("\n".join(text) + "\n")
print(f"wrote {path}: 2 x {NSLOT} slots, cap {CAP} cycles; (max VALU cycles per slot, total VALU cycles, commits done by slot, cycles over the cap, "
      f"pool done by slot): {[(round(a, 1), round(b), c, round(d), e) for a, b, c, d, e in stats]}")
