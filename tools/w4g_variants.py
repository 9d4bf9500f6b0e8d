#!/usr/bin/env python3
"""Where the F(4x4) GEMM kernel's time goes: textual variants of the shipping
csrc/conv_winograd4.hip (tools only, never shipped), each linked with tools/w4g_bench.cpp.

A variant edits the source at anchors named after the kernel's roles and helpers
(the three branches of wino4_body, half_patch_to_ring, ring_put, load_residual8, launch_wino4).  Every anchor must occur exactly once (sub()): a stale anchor
fails loudly.  Variants whose anchors left the kernel in earlier rounds are gone; what they
measured is in DESIGN.md sections 4 and 5.

usage: w4g_variants.py build [names...]   (here, hipcc cross-compiles)
       w4g_variants.py run [names...]     (on the GPU box)
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "facerecognitionpipeline_amd", "csrc")
SRC = os.path.join(CSRC, "conv_winograd4.hip")
BENCH = os.path.join(REPO, "tools", "w4g_bench.cpp")
OUT = os.path.join(REPO, "tools", "wv")
SHAPES = [(256, 14, 256, 256, 2), (256, 14, 256, 256, 1), (256, 28, 128, 128, 2), (256, 56, 64, 64, 2),
          (256, 7, 512, 512, 2)]


def sub(s, anchor, new):
    """replace the one occurrence of anchor"""
    assert s.count(anchor) == 1, (s.count(anchor), anchor[:80])
    return s.replace(anchor, new)


def subs(s, *pairs):
    for anchor, new in pairs:
        s = sub(s, anchor, new)
    return s


def chain(*fs):
    def f(s):
        for g in fs:
            s = g(s)
        return s
    return f


# ---- the transform waves (default item / wide and tall items) ----
DEF_PUT = "      ring_put<NMW, NBUF>(fre, rdy, t, lane, g, fseen, p.poll_max, [&] { store(P, g); });\n"
SHAPED_PUT = "        ring_put<NMW, NBT>(fre, rdy, t, lane, g, fseen, p.poll_max, [&] { store(P, g); });\n"
DEF_LOAD = "          const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, poff[a][b], soff, 0);"
SHAPED_LOAD = "              const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(xr, poff[q][a][b], soff, 0);"
PRE_PRIO = "    if constexpr (PRE) __builtin_amdgcn_s_setprio(1);\n"
DEF_T = "    const int t = wid - 4;\n"


def def_store(new):
    """the default transform waves' put with `new` in place of store(P, g)"""
    return lambda s: sub(s, DEF_PUT, DEF_PUT.replace("store(P, g);", new))


def noload(s):
    """no patch loads: the offsets stand in for the data"""
    return subs(s, (DEF_LOAD, "          const u32x2 v = {(unsigned)(poff[a][b] + soff), 0u};"),
                (SHAPED_LOAD, "              const u32x2 v = {(unsigned)(poff[q][a][b] + soff), 0u};"))


def notrans(s):
    """the transform waves keep loading and publishing, but transform and write nothing"""
    return subs(s, (DEF_PUT, DEF_PUT.replace("{ store(P, g); }", "{}")), (SHAPED_PUT, SHAPED_PUT.replace("{ store(P, g); }", "{}")))


def waitonly(s):
    """the default transform waves wait for their patch loads (one sum of the patch written to the
    ring), but run none of the transform's arithmetic: separates the patch-load latency from the
    transform code's cost"""
    return def_store("""
        f2 sm = P.d[0][0];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) sm += P.d[a][b];
        *reinterpret_cast<f2*>(ring + (g % NBUF) * VSTEP + dst_off) = sm;
     """)(s)


def halftrans(s):
    """transform + LDS writes on even K-steps only (wrong results): the gain an item with twice
    the couts per transformed patch could reach"""
    return def_store("if ((g & 1) == 0) store(P, g);")(s)


def halfpatch(s):
    """halftrans + patch loads of odd K-steps skipped"""
    s = sub(s, DEF_LOAD, "          const u32x2 v = (ls & 1) ? u32x2{0u, 0u} : __builtin_amdgcn_raw_buffer_load_b64(r, poff[a][b], soff, 0);")
    return halftrans(s)


def noenter(s):
    """geometry of the first item only (outputs wrong): what enter_item costs per item"""
    a = "      ks_real = steps_of(it);\n      step0 = SPLIT ? it.split * KS : 0;\n"
    return sub(s, a, a + "      if (j > 0) return;\n")


def prio_tr(s):
    """transform waves (the younger half, waves 4-7) at s_setprio 1"""
    return sub(s, DEF_T, DEF_T + "    __builtin_amdgcn_s_setprio(1);\n")


def noprio(s):
    return sub(s, PRE_PRIO, "")


def aprio(s, ahead=1):
    """transform waves at issue priority only while the ring holds <= 1 transformed step ahead of
    the slowest MFMA wave (else priority 0), for every epilogue"""
    s = sub(s, PRE_PRIO, "")
    return sub(s, DEF_PUT, "      {\n        const int ahead = g - lds_min<4>(fre);\n"
                           f"        if (ahead <= {ahead}) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);\n"
                           "      }\n" + DEF_PUT)


def aprio2(s):
    """aprio with the threshold at 2 steps ahead"""
    return aprio(s, 2)


LOOP3 = """    Patch pa, pb, pc;"""
LOOPBODY3 = """    load(pa);
    load(pb);
    for (int b = 0;; b += 3) {
      load(pc);
      __builtin_amdgcn_sched_barrier(0);  // the loads go out first
      put(pa, b);
      if (b + 1 >= G) break;
      load(pa);
      __builtin_amdgcn_sched_barrier(0);
      put(pb, b + 1);
      if (b + 2 >= G) break;
      load(pb);
      __builtin_amdgcn_sched_barrier(0);
      put(pc, b + 2);
      if (b + 3 >= G) break;
    }"""
LOOPBODY4 = """    load(pa);
    load(pb);
    load(pc);
    for (int b = 0;; b += 4) {
      load(pd);
      __builtin_amdgcn_sched_barrier(0);  // the loads go out first
      put(pa, b);
      if (b + 1 >= G) break;
      load(pa);
      __builtin_amdgcn_sched_barrier(0);
      put(pb, b + 1);
      if (b + 2 >= G) break;
      load(pb);
      __builtin_amdgcn_sched_barrier(0);
      put(pc, b + 2);
      if (b + 3 >= G) break;
      load(pc);
      __builtin_amdgcn_sched_barrier(0);
      put(pd, b + 3);
      if (b + 4 >= G) break;
    }"""


def pf3(s):
    """patch loads three K-steps ahead (four rotating buffers) instead of two"""
    return subs(s, (LOOP3, "    Patch pa, pb, pc, pd;"), (LOOPBODY3, LOOPBODY4))


PLOAD = """#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, poff[a][b], soff, 0);
          P.d[a][b] = f2{__uint_as_float(v.x), __uint_as_float(v.y)};
        }"""
PLOAD12 = """#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, poff[a][0], soff, 0);
        P.d[a][0] = f2{__uint_as_float(v.x), __uint_as_float(v.y)};
        P.d[a][1] = f2{__uint_as_float(v.z), __uint_as_float(v.w)};
        const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(r, poff[a][2], soff, 0);
        P.d[a][2] = f2{__uint_as_float(w.x), __uint_as_float(w.y)};
      }"""


def load12(s):
    """12 patch loads per lane and step (6 of them 16-byte) instead of 18 8-byte ones, same bytes
    give or take (wrong data): does the load instruction count or the bytes cost?"""
    return sub(s, PLOAD, PLOAD12)


# ---- the MFMA waves ----
MFMA_HEAD = "  // ---- MFMA waves: wave w owns couts 16w .. 16w+15 of every item"
MFMA8 = "".join(f"        acc[x{o}] = __builtin_amdgcn_mfma_f32_16x16x4f32(u{e}.{c}, a{e}.{c}, acc[x{o}], 0, 0, 0);\n"
                for c in "xyzw" for e, o in ((0, ""), (1, " + 1")))
ULOAD = """          uring[y % URING] = y + URING < NXI ? ld4(ur, lo, (y + URING) * XS + cur)
                                             : ld4(ur, lo, (y + URING - NXI) * XS + nxt);"""
EPI_START = "    // an idle quarter (!live, Cout % 64 != 0) runs the epilogue too"
EPI_END = "  };\n  for (; j < nloc; ++j) segment();\n"
URING_DEPTH = "  return (EPI == EPI_AFFINE_RES || EPI == EPI_AFFINE_RES_PRELU) ? 9 : 12;"
PARTB_STORE = "    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 0);\n"
PARTB_CALL = "          if (x >= 4) finish(x / 2 - 2);"
YR_D = "  const __amdgpu_buffer_rsrc_t yr_d = uniform_rsrc(p.y, p.B * H * W * Cout * 4);\n"


def nomfma(s):
    return sub(s, MFMA8, "        acc[x][0] += a0.x * u0.x + a1.w * u1.w;\n")


def nouload(s):
    return sub(s, ULOAD, "")


def halfu(s):
    """U refills of odd xi skipped (wrong results): the gain of twice the tiles per U fragment"""
    a = "          uring[y % URING] = y + URING < NXI ?"
    return sub(s, a, "          if (e == 0) uring[y % URING] = y + URING < NXI ?")


def noepi(s):
    """no epilogue: one sum of the accumulators keeps the MFMAs alive"""
    assert s.count(EPI_START) == 1 and s.count(EPI_END) == 1
    a = s.index(EPI_START)
    b = s.index(EPI_END, a)
    dummy = ("    float sum = 0.f;\n#pragma unroll\n    for (int x = 0; x < NXI; ++x) sum += acc[x][0] + acc[x][3];\n"
             "    if (sum == 12345.f) p.y[lane] = 1.f;\n")
    return s[:a] + dummy + s[b:]


def prio_mfma(s):
    """MFMA waves at s_setprio 1: they win issue arbitration on their SIMD"""
    return sub(s, MFMA_HEAD, "  __builtin_amdgcn_s_setprio(1);\n" + MFMA_HEAD)


def uring(res, other):
    return lambda s: sub(s, URING_DEPTH, f"  return (EPI == EPI_AFFINE_RES || EPI == EPI_AFFINE_RES_PRELU) ? {res} : {other};")


def upolicy(aux):
    """U fragment loads with a cache-policy aux field (sc0 = 1, nt = 2, sc1 = 16): L1 bypass"""
    def f(s):
        ld4_def = "__device__ __forceinline__ f4 ld4(__amdgpu_buffer_rsrc_t r, int off, int soff = 0) {"
        extra = ("template <int AUX>\n__device__ __forceinline__ f4 ld4p(__amdgpu_buffer_rsrc_t r, int off, int soff = 0) {\n"
                 "  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, AUX);\n"
                 "  return f4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};\n}\n\n")
        s = sub(s, ld4_def, extra + ld4_def)
        for a in ("uring[r] = ld4(ur, ", "? ld4(ur, ", ": ld4(ur, "):
            s = sub(s, a, a.replace("ld4(", f"ld4p<{aux}>("))
        return s
    return f


def partb(new):
    return lambda s: sub(s, PARTB_STORE, new)


def nopartb(s):
    return sub(s, PARTB_CALL, "          if (x >= 4 && p.B < 0) finish(x / 2 - 2);")


def y2store(s):
    """conv2 epilogues also write BN_next(y) = y * s + t (here the post-BN pair again) into a second
    tensor of y's shape (the residual buffer: timing only): what the next conv1's pre-BN costs here"""
    s = sub(s, PARTB_STORE, PARTB_STORE + """    if constexpr (DRES) {
      const f4 v2 = __builtin_elementwise_fma(v, psc, psh);
      const u32x4 b2 = {__float_as_uint(v2.x), __float_as_uint(v2.y), __float_as_uint(v2.z), __float_as_uint(v2.w)};
      __builtin_amdgcn_raw_buffer_store_b128(b2, y2r_d, po[i], 0, 0);
    }
""")
    return sub(s, YR_D, YR_D + "  const __amdgpu_buffer_rsrc_t y2r_d = uniform_rsrc(p.res, p.res ? p.B * H * W * Cout * 4 : 0);\n")


FINISH = """  auto finish = [&](int i) {  // part B of pending pixel i
    f4 v = __builtin_elementwise_fma(pv[i], psc, psh);
    if constexpr (EPI == EPI_AFFINE_PRELU) v = prelu_q(v, pal, pcl);
    if constexpr (DRES) {
      v += pres[i];
      if constexpr (EPI == EPI_AFFINE_RES_PRELU) v = prelu_q(v, pal, pcl);
    }
    const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 0);
  };
"""
PAIRSTORE = """  // part B in pixel pairs (x, x + 1) of a tile row: lanes of tiles n, n ^ 1 (lane ^ 1, same couts)
  // swap one value each (DPP quad_perm [1,0,3,2]) so that each store instruction writes whole
  // 128-B lines of the channel-blocked output (pixels 2k, 2k + 1 of one tile)
  f4 pend = {0.f, 0.f, 0.f, 0.f};
  int pend_off = BIGOFF;
  auto epi_px = [&](int i) {
    f4 v = __builtin_elementwise_fma(pv[i], psc, psh);
    if constexpr (EPI == EPI_AFFINE_PRELU) v = prelu_q(v, pal, pcl);
    if constexpr (DRES) {
      v += pres[i];
      if constexpr (EPI == EPI_AFFINE_RES_PRELU) v = prelu_q(v, pal, pcl);
    }
    return v;
  };
  auto swp = [](float f) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(f), 0xB1, 0xF, 0xF, false));
  };
  auto st = [&](f4 v, int off) {
    const u32x4 bits = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, off, 0, 0);
  };
  auto finish = [&](int i) {
    if ((i & 1) == 0) {
      const bool odd = (threadIdx.x & 1) != 0;
      const f4 v0 = epi_px(i), v1 = epi_px(i + 1);
      const f4 t = odd ? v0 : v1;
      const f4 sw = {swp(t.x), swp(t.y), swp(t.z), swp(t.w)};
      const int so = __builtin_amdgcn_update_dpp(0, odd ? po[i] : po[i + 1], 0xB1, 0xF, 0xF, false);
      st(odd ? sw : v0, odd ? so : po[i]);
      pend = odd ? v1 : sw;
      pend_off = odd ? po[i + 1] : so;
    } else {
      st(pend, pend_off);
    }
  };
"""


def pairstore(s):
    return sub(s, FINISH, PAIRSTORE)


AT6V = """  const f2 c2 = {2.f, 2.f}, c4 = {4.f, 4.f}, c8 = {8.f, 8.f};
  const f2 p12 = m[1] + m[2], m12 = m[1] - m[2];
  const f2 p34 = m[3] + m[4], m34 = m[3] - m[4];
  o[0] = m[0] + p12 + p34;
  o[1] = __builtin_elementwise_fma(c2, m34, m12);
  o[2] = __builtin_elementwise_fma(c4, p34, p12);
  o[3] = __builtin_elementwise_fma(c8, m34, m12 + m[5]);"""
AT6S = """#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float p12 = m[1][e] + m[2][e], m12 = m[1][e] - m[2][e];
    const float p34 = m[3][e] + m[4][e], m34 = m[3][e] - m[4][e];
    o[0][e] = m[0][e] + p12 + p34;
    o[1][e] = __builtin_fmaf(2.f, m34, m12);
    o[2][e] = __builtin_fmaf(4.f, p34, p12);
    o[3][e] = __builtin_fmaf(8.f, m34, m12 + m[5][e]);
  }"""


def scalarepi(s):
    """the two-cout output transform (at6v) in scalar f32 (same arithmetic per element)"""
    return sub(s, AT6V, AT6S)


# ---- per-wave cycle accounting ----
STAMP_HDR = """
// ---- stamps variant: per-wave cycle accounting (s_memtime), written once per wave by lane 0 ----
__device__ unsigned long long w4dbg[1024 * 8 * 4];
#define W4_PUT()                                                                        \\
  if (lane == 0) {                                                                      \\
    unsigned long long* d_ = w4dbg + ((size_t)bid * 8 + wid) * 4;                       \\
    d_[0] = __builtin_amdgcn_s_memtime() - t_start;                                     \\
    d_[1] = 0;                                                                          \\
    d_[2] = epi_cyc;                                                                    \\
    d_[3] = (unsigned long long)G;                                                      \\
  }
"""
STAMP_HOST = """
#include <cstdio>
extern "C" void w4g_after_run() {
  static unsigned long long h[1024 * 8 * 4];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(frhip::w4dbg), sizeof(h)) != hipSuccess) return;
  double tot[2] = {0, 0}, epi[2] = {0, 0}, st[2] = {0, 0};
  unsigned long long tmax[2] = {0, 0};
  int n[2] = {0, 0};
  for (int b = 0; b < 1024; ++b)
    for (int w = 0; w < 8; ++w) {
      const unsigned long long* d = h + ((size_t)b * 8 + w) * 4;
      if (!d[0]) continue;
      const int k = w < 4 ? 0 : 1;
      tot[k] += d[0]; epi[k] += d[2]; st[k] += d[3]; ++n[k];
      if (d[0] > tmax[k]) tmax[k] = d[0];
    }
  for (int k = 0; k < 2; ++k)
    if (n[k])
      printf("  %s waves: %d, avg total %.0f cyc (max %llu), epilogue %.0f (%.1f%%), "
             "K-steps %.1f -> %.0f cyc/K-step, %.0f outside the epilogue per K-step\\n",
             k ? "transform" : "MFMA", n[k], tot[k] / n[k], tmax[k], epi[k] / n[k], 100 * epi[k] / tot[k], st[k] / n[k],
             tot[k] / st[k], (tot[k] - epi[k]) / st[k]);
}
"""
STAMP_START = ("  unsigned long long epi_cyc = 0;\n"
               "  const unsigned long long t_start = __builtin_amdgcn_s_memtime();\n")


def stamps(s):
    """s_memtime accounting per wave of the default transform waves and the MFMA waves: total and the
    MFMA-wave epilogue (part A; part B runs inside the next item's MFMAs)"""
    a = "__device__ __forceinline__ int canvas_coord("
    s = sub(s, a, STAMP_HDR + a)
    a = "  const int tid = threadIdx.x, lane = tid & 63;\n"
    s = sub(s, a, a + STAMP_START)
    a = "      if (b + 3 >= G) break;\n    }\n    w4_report_handoff(fseen, p.err);\n    return;"
    s = sub(s, a, "      if (b + 3 >= G) break;\n    }\n    W4_PUT();\n    w4_report_handoff(fseen, p.err);\n    return;")
    s = sub(s, EPI_START, "    const unsigned long long t_e0 = __builtin_amdgcn_s_memtime();\n" + EPI_START)
    a = "      transform_to_pv();\n      set_pending();\n      return;"
    s = sub(s, a, "      transform_to_pv();\n      set_pending();\n      epi_cyc += __builtin_amdgcn_s_memtime() - t_e0;\n      return;")
    a = "  w4_report_handoff(rseen, p.err);\n}\n"
    s = sub(s, a, "  W4_PUT();\n  w4_report_handoff(rseen, p.err);\n}\n")
    return s + STAMP_HOST


# ---- the host side (launch_wino4) ----
NBG = "  p.nbg = std::max(1, std::min(p.mblocks, std::max(32 / p.nblocks, 8)));"
LAUNCH = "hipError_t launch_wino4(const Wino4Params& p0, bool pre, Epi epi, hipStream_t s) {\n"


def nbg(minimum):
    """at least `minimum` tile blocks per XCD item group (Cout = 512: 4 -> 8, U streamed per XCD
    round halves, patches read twice)"""
    return lambda s: sub(s, NBG, f"  p.nbg = std::max(1, std::min(p.mblocks, std::max(32 / p.nblocks, {minimum})));")


def nopre(s):
    """conv1 without the pre-BN in the transform (as if the previous conv2's epilogue had applied it
    to a second copy of its output): timing only"""
    return subs(s, (LAUNCH, LAUNCH + "  if (pre && epi == EPI_AFFINE_PRELU) pre = false;\n"),
                ("    {true, EPI_AFFINE_PRELU, 0, 0, 0, wino4_kernel<true, EPI_AFFINE_PRELU, 0>, nullptr},\n", ""),
                ("    {true, EPI_AFFINE_PRELU, 1, 0, 0, wino4_kernel<true, EPI_AFFINE_PRELU, 1>, wino4_part_fixup_kernel<EPI_AFFINE_PRELU>},\n", ""))


def nofixup(s):
    return sub(s, "    if (in.fixup)  // 64-thread blocks", "    if (false)  // 64-thread blocks")


VARIANTS = {
    "base": lambda s: s,
    # where the time goes: pieces removed (wrong results, timing only)
    "noload": noload,
    "notrans": notrans,
    "nomfma": nomfma,
    "nouload": nouload,
    "noepi": noepi,
    "mfmaonly": chain(noepi, notrans, nouload),
    "skeleton": chain(nomfma, noepi, notrans, nouload),
    "nomfma_noload": chain(nomfma, noload),
    "nomfma_notrans": chain(nomfma, notrans),
    "nomfma_noepi": chain(nomfma, noepi),
    "waitonly": waitonly,
    "noenter": noenter,
    "halftrans": halftrans,
    "halfpatch": halfpatch,
    "halfu": halfu,
    "load12": load12,
    "nofixup": nofixup,
    # deferred epilogue pieces removed (wrong results, timing only)
    "nopartb": nopartb,
    "nores2": lambda s: sub(s, "pres[i] = ld4(rr, oo[i >> 2][i & 3]);", "pres[i] = f4{0.f, 0.f, 0.f, 0.f};"),
    "partb_nostore": partb("    if (v.x == 12345.678f && p.B < 0) __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 0);\n"),
    "partb_small": partb("    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i] & 0xfff0, 0, 0);\n"),
    # schedule, layout and cache-policy experiments
    "pairstore": pairstore,
    "nopre": nopre,
    "y2store": y2store,
    "uring18pre": uring(9, 18),
    "uring6res": uring(6, 12),
    "u18split": lambda s: sub(s, "  constexpr int URING = uring_depth<EPI>();", "  constexpr int URING = MODE == 1 ? 18 : uring_depth<EPI>();"),
    "nbg16": nbg(16),
    "nbuf3": lambda s: sub(s, "constexpr int NBUF = 4; ", "constexpr int NBUF = 3; "),
    "pf3": pf3,
    "u_sc1": upolicy(16),
    "u_nt": upolicy(2),
    "u_sc01": upolicy(17),
    "u_sc0": upolicy(1),
    "partb_sc1": partb("    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 16);\n"),
    "partb_sc0": partb("    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 1);\n"),
    "partb_sc01": partb("    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 17);\n"),
    "partb_nt": partb("    __builtin_amdgcn_raw_buffer_store_b128(bits, yr_d, po[i], 0, 2);\n"),
    "prio_mfma": prio_mfma,
    "prio_tr": prio_tr,
    "noprio": noprio,
    "aprio": aprio,
    "aprio2": aprio2,
    "scalarepi": scalarepi,
    # cycle stamps
    "stamps": stamps,
    "stamps_prio_mfma": chain(prio_mfma, stamps),
    "stamps_prio_tr": chain(prio_tr, stamps),
    "stamps_nopartb": chain(nopartb, stamps),
}


def build(name):
    s = open(SRC).read()
    v = VARIANTS[name](s)
    assert name == "base" or v != s, name
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(OUT, f"w4g_{name}.hip")
    open(src, "w").write(v)
    exe = os.path.join(OUT, f"w4g_{name}")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I" + CSRC,
                    "-I" + os.path.join(REPO, "include"), "-x", "hip", src, "-x", "hip", BENCH, "-o", exe], check=True)
    return exe


def main():
    cmd, names = sys.argv[1], sys.argv[2:] or list(VARIANTS)
    if cmd == "build":
        with ThreadPoolExecutor(8) as ex:
            print(list(ex.map(build, names)))
    else:
        for n in names:
            # base: the default schedule (whole items + tail split-K), whole items only, stream-K
            for tag, sk, ns in ((("", 0, 0), ("/whole", 0, 1), ("/sk", 2, 0)) if n == "base" else (("", 0, 0),)):
                for shp in SHAPES:
                    r = subprocess.run(["timeout", "-k", "5", "60", os.path.join(OUT, f"w4g_{n}")] +
                                       [str(x) for x in shp] + ["20", str(sk), str(ns)], capture_output=True, text=True)
                    print(f"{n + tag:12s} {r.stdout.strip()} {r.stderr.strip()[-200:]}", flush=True)
                    if r.returncode:
                        return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
