"""Case table of tests/test_footprint_gpu.py for mdx_gemm_f16 (dense GEMMs and convs), kept free of any device access so that
tests/test_footprint_cpu.py can resolve every row on the host (mdx_gemm_check / mdx_gemm_query) and build the coverage matrix.

A case is a dict (see `case()` for the fields).  `form` names the launch form the case means to test; what mdx_gemm_query must
report for it is derived in `expected_query()`.  Shapes are the smallest at which each tail exists.

Replacements of descriptors the library refuses (the nearest accepted one is used instead):
  * two sources with c2 = 8: "two-source input needs c1 % 64 == 0 and Cin % 64 == 0" -> c1 = 64, c2 = 64;
  * the sub-pixel form at N = 72: the sub-pixel weights are packed per parity in whole 64-row panels (N % 64 == 0) -> N = 64;
  * MDX_OUT_TRANSPOSED with the LayerNorm fold: "LayerNorm fold needs ... a dense row-major GEMM" -> the fold rides on the n_split
    launches only (their launch is row-major; the V^T columns go through the same transposed store);
  * the lean dense kernel takes K tiles of whole 64-channel chunks and the plain / GEGLU epilogues: its rows use K = 320 and no
    activation; K in {8, 72} and GELU / QuickGELU / PReLU are carried by the generic kernel;
  * split 5 needs five K tiles: K = 320; split 2 needs two: K in {72, 320};
  * a HALO split owns whole 64-channel chunks: split 2 runs at Cin = 128, split 3 at Cin = 192, split 5 at Cin = 320.
"""
EPI = {"none": 0, "geglu": 1, "gelu": 2, "qgelu": 3, "prelu": 4}
MODE = {"row": 0, "T": 1, "d2s": 2}
FORMS = ("generic", "halo", "halo8", "wfrag", "conv8p", "subpix", "lean", "t160")


def case(cid, form, B, H, W, c1, N, **kw):
    c = dict(id=cid, form=form, B=B, H=H, W=W, c1=c1, c2=0, N=N, ks=1, stride=1, up=0, asym=0, epi="none", mode="row", splitk=1,
             tile_m=0, tile_n=0, stages=0, lean=None, ld_extra=8, bias=True, rowbias=False, residual=False, stats_out=False,
             lnfold=False, colstats=False, n_split=0, ctx=0, w_frag=0, skip=0, w_sub=False, geglu_unit=0, tol=1e-3)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


def out_hw(c):
    Hs, Ws = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    lo = (0 if c["asym"] else 1) if c["ks"] == 3 else 0
    hi = 1 if c["ks"] == 3 else 0
    return (Hs + lo + hi - c["ks"]) // c["stride"] + 1, (Ws + lo + hi - c["ks"]) // c["stride"] + 1


def width(c):
    """Logical columns of the row-major output (the d2s pixel's channels; the q|k part of an n_split launch)."""
    if c["mode"] == "d2s":
        return c["N"] // 4
    if c["n_split"]:
        return c["n_split"]
    return c["N"] // 2 if c["epi"] == "geglu" else c["N"]


def out_ld(c):
    if c["mode"] == "T":
        Ho, Wo = out_hw(c)
        return c["ctx"] + (Ho * Wo + 7) // 8 * 8 + 8      # [B][N][ctx + tokens, padded]: the next multiple of 8 plus 8
    return width(c) + c["ld_extra"]


def expected_query(c):
    """Fields of mdx_gemm_query (index -> value) this case must resolve to."""
    e = {}
    if c["tile_m"]:
        e[0] = c["tile_m"]
    if c["tile_n"]:
        e[1] = c["tile_n"]
    form = c["form"]
    e[3] = {"generic": 0, "lean": 2, "t160": 2}.get(form, 1)
    if form == "t160":
        e[0], e[1] = 128, 160
    if form in ("halo", "halo8", "wfrag"):
        e[0] = 128
    if form in ("conv8p", "subpix"):
        e[0], e[2] = 256, 1
    else:
        if c["splitk"]:
            e[2] = c["splitk"]
        if c["splitk"] > 1:
            e[6] = 1 if (c["splitk"] <= 4 and c["mode"] != "T") else 0
    return e


def make_desc(ops, c, t):
    """The descriptor of case c over the tensors t[name] (name -> tensor; anything that returns a tensor for a name serves)."""
    Ho, Wo = out_hw(c)
    kw = dict(ksize=c["ks"], stride=c["stride"], upsample=c["up"], asym_pad=c["asym"], epilogue=EPI[c["epi"]],
              out_mode=MODE[c["mode"]], splitk=c["splitk"], tile_m=c["tile_m"], tile_n=c["tile_n"], stages=c["stages"],
              w_frag=c["w_frag"], geglu_unit=c["geglu_unit"])
    if c["c2"]:
        kw.update(a2=t["a2"], c2=c["c2"])
    if c["bias"]:
        kw["bias"] = t["bias"]
    if c["rowbias"]:
        kw.update(rowbias=t["rowbias"], rowbias_ld=c["N"] + 12)
    if c["residual"]:
        kw.update(residual=t["residual"], residual_ld=width(c) + 16)
    if c["stats_out"]:
        kw["stats_out"] = t["stats_out"]
    if c["lnfold"]:
        kw.update(ln_stats=t["ln_stats"], ln_s=t["ln_s"], ln_eps=1e-5)
    if c["epi"] == "prelu":
        kw["act_slope"] = t["act_slope"]
    if c["skip"]:
        kw.update(skip_a=t["skip_a"], skip_c1=c["skip"], skip_w=t["skip_w"])
    if c["w_sub"]:
        kw["w_sub"] = t["w_sub"]
    if c["n_split"]:
        kw.update(n_split=c["n_split"], out2=t["out2"], out2_ld=c["ctx"] + Ho * Wo, out_bs=(c["ctx"] + Ho * Wo) * out_ld(c))
    d = ops.make_gemm_desc(t["a"], t["w"], c["N"], c["B"], c["H"], c["W"], c["c1"], t["out"], out_ld(c), **kw)
    if c["epi"] == "prelu":
        d.act_slope_n = width(c) if c["mode"] == "d2s" else c["N"]
    if c["colstats"] and "colstats_out" in t:      # (its size follows from the rows per block mdx_gemm_query reports: set by the caller)
        d.colstats_out = t["colstats_out"].data_ptr()
    return d


# ----------------------------------------------------------------------------------------------------------- the table
def _dense():
    rows = []
    Ms, Ns, Ks = [1, 63, 65, 129, 200], [8, 72, 136, 192], [8, 72, 320]
    epis = ["none", "gelu", "qgelu", "prelu"]
    i = 0
    for lean in (0, 1):
        for tm in (64, 128):
            for tn in (64, 128):
                for sk in (1, 2, 5):
                    M, N = Ms[i % 5], Ns[i % 4]
                    K = 320 if (lean or sk == 5) else (Ks[i % 3] if sk == 1 else (72, 320)[i % 2])
                    epi = "none" if lean else epis[i % 4]
                    if epi == "prelu" and K % 64:
                        K = 320      # PReLU launches take Cin % 64 == 0
                    rows.append(case(f"dense_{'lean' if lean else 'gen'}_{tm}x{tn}_s{sk}_M{M}_N{N}_K{K}_{epi}",
                                     "lean" if (lean and sk <= 4) else "generic",      # (a split past the ticket limit leaves the lean kernel)
                                     1, M, 1, K, N, lean=lean, tile_m=tm, tile_n=tn, splitk=sk, epi=epi, ld_extra=(8, 24)[i % 2],
                                     residual=epi in ("none", "prelu"), rowbias=(not lean) and epi == "none"))
                    i += 1
    # every M, N and K of the issue appears at least once on each kernel's unsplit auto-tile launch as well
    for j, (M, N, K) in enumerate([(1, 8, 8), (63, 72, 72), (65, 136, 320), (129, 192, 8), (200, 8, 72), (1, 192, 320), (200, 136, 72)]):
        rows.append(case(f"dense_gen_auto_M{M}_N{N}_K{K}", "generic", 1, M, 1, K, N, lean=0, ld_extra=(24, 8)[j % 2], residual=True,
                         rowbias=True))
    for j, (M, N) in enumerate([(1, 72), (63, 192), (65, 8), (129, 136), (200, 72)]):
        rows.append(case(f"dense_lean_auto_M{M}_N{N}_K320", "lean", 1, M, 1, 320, N, lean=1, ld_extra=(24, 8)[j % 2], residual=True))
    # GEGLU: N = 256 (128 produced columns) at unit 64 on both kernels, N = 320 at unit 80 on the 128 x 160 tile
    rows.append(case("geglu_gen_M100_N256_u64", "generic", 1, 100, 1, 72, 256, lean=0, epi="geglu", tol=2e-3))
    rows.append(case("geglu_lean_M100_N256_u64", "lean", 1, 100, 1, 320, 256, lean=1, epi="geglu", geglu_unit=64, tol=2e-3))
    rows.append(case("geglu_t160_M100_N320_u80", "t160", 1, 100, 1, 320, 320, lean=1, epi="geglu", geglu_unit=80, tile_m=128,
                     tile_n=160, tol=2e-3, ld_extra=24))
    # the 128 x 160 tile with an N tail (200 = 160 + 40) and an M tail, bias + residual
    rows.append(case("t160_M129_N200", "t160", 1, 129, 1, 320, 200, lean=1, tile_m=128, tile_n=160, residual=True))
    # LayerNorm fold: row-statistics producer and consumer, N = 64 and 320, M = 200
    for N in (64, 320):
        for lean in (0, 1):
            f = "lean" if lean else "generic"
            rows.append(case(f"stats_producer_{f}_N{N}", f, 1, 200, 1, 320 if lean else 72, N, lean=lean, residual=True, stats_out=True))
            rows.append(case(f"lnfold_consumer_{f}_N{N}", f, 1, 200, 1, 64 if N == 320 else 320, N, lean=lean, lnfold=True, tol=2e-3))
        rows.append(case(f"lnfold_consumer_lean_N{N}_s2", "lean", 1, 200, 1, 320, N, lean=1, lnfold=True, splitk=2, tol=2e-3, ld_extra=24))
    rows.append(case("lnfold_consumer_t160_N320", "t160", 1, 200, 1, 64, 320, lean=1, lnfold=True, tile_m=128, tile_n=160, tol=2e-3))
    # column statistics: tokens per sample = one tile and two tiles (cap = exactly the row blocks produced)
    for T in (128, 256):
        for lean in (0, 1):
            rows.append(case(f"colstats_{'lean' if lean else 'gen'}_T{T}", "lean" if lean else "generic", 2, T, 1, 64, 72, lean=lean,
                             tile_m=128, colstats=True))
    return rows


def _transposed():
    rows = []
    for i, T in enumerate((25, 49, 64, 80)):
        for sk in (1, 3):
            rows.append(case(f"transposed_T{T}_s{sk}", "generic", 2, T, 1, 320 if sk == 3 else 64, (128, 72)[i % 2], mode="T", ctx=8,
                             splitk=sk))
    for T in (64, 80):
        for sk in (1, 3):
            for fold in (False, True):
                rows.append(case(f"nsplit_T{T}_s{sk}_ln{int(fold)}", "generic", 2, T, 1, 192, 384, n_split=256, ctx=16, splitk=sk, lnfold=fold,
                                 tol=2e-3 if fold else 1e-3, lean=0))
    return rows


def _convs():
    rows = []
    g = dict(ks=3, lean=None)
    rows.append(case("conv_gen_6x10_N72", "generic", 2, 6, 10, 64, 72, **g, rowbias=True, residual=True))
    rows.append(case("conv_gen_s2_7x9", "generic", 2, 7, 9, 64, 72, stride=2, **g))
    rows.append(case("conv_gen_s2_16x16", "generic", 2, 16, 16, 64, 136, stride=2, **g, ld_extra=24))
    rows.append(case("conv_gen_asym_16x16", "generic", 2, 16, 16, 64, 72, stride=2, asym=1, **g))
    rows.append(case("conv_gen_asym_7x9", "generic", 2, 7, 9, 64, 72, stride=2, asym=1, **g))
    rows.append(case("conv_gen_upsample_5x6", "generic", 2, 5, 6, 64, 72, up=1, **g))
    rows.append(case("conv_gen_two_sources", "generic", 2, 6, 10, 64, 72, c2=64, **g))      # (c2 = 8 is refused: see the module docstring)
    rows.append(case("conv_gen_cin8", "generic", 2, 6, 10, 8, 72, **g))                     # tap-major K order, K = 72
    rows.append(case("conv_gen_6x10_s2k", "generic", 2, 6, 10, 128, 72, **g, splitk=2))
    rows.append(case("conv_gen_6x10_s5k", "generic", 2, 6, 10, 64, 72, **g, splitk=5, ld_extra=24))
    # HALO 8 x 16 patches
    i = 0
    for (H, W) in ((8, 16), (16, 32)):
        for N in (72, 192):
            for B in (1, 3):
                for sk in (1, 2):
                    rows.append(case(f"halo_{H}x{W}_N{N}_B{B}_s{sk}", "halo", B, H, W, 128, N, **g, splitk=sk, ld_extra=(8, 24)[i % 2],
                                     rowbias=i % 2 == 0, residual=i % 4 < 2))
                    i += 1
    rows.append(case("halo_8x16_N72_B3_s5", "halo", 3, 8, 16, 320, 72, **g, splitk=5))
    rows.append(case("halo_16x16_colstats", "halo", 2, 16, 16, 64, 72, **g, colstats=True))
    rows.append(case("halo_16x16_fused_skip", "halo", 2, 16, 16, 64, 72, **g, skip=64, residual=True))
    # HALO8: two 8 x 8 samples per 128-row tile; odd batches leave the last tile half empty
    for B in (1, 3, 5):
        for (cin, sk) in ((64, 1), (192, 1), (192, 3)):
            for N in (64, 72):
                rows.append(case(f"halo8_B{B}_C{cin}_N{N}_s{sk}", "halo8", B, 8, 8, cin, N, **g, splitk=sk, rowbias=True, residual=True,
                                 ld_extra=(8, 24)[(B // 2 + N // 8) % 2]))
    rows.append(case("halo8_B3_C320_N72_s5", "halo8", 3, 8, 8, 320, 72, **g, splitk=5, rowbias=True, residual=True))
    # weight-streaming form (fragment-major weights, 128-row HALO tiles)
    rows.append(case("wfrag_B2_8x8_N64", "wfrag", 2, 8, 8, 64, 64, **g, w_frag=1, tile_m=128))
    rows.append(case("wfrag_B3_8x8_N128", "wfrag", 3, 8, 8, 128, 128, **g, w_frag=1, tile_m=128, splitk=2, ld_extra=24))
    rows.append(case("wfrag_B1_16x16_N64", "wfrag", 1, 16, 16, 128, 64, **g, w_frag=1, tile_m=128, residual=True))
    rows.append(case("wfrag_B2_16x16_N192_tn128", "wfrag", 2, 16, 16, 64, 192, **g, w_frag=1, tile_m=128, tile_n=128))      # N tail: 192 = 128 + 64
    rows.append(case("wfrag_B1_16x16_N128_s5", "wfrag", 1, 16, 16, 320, 128, **g, w_frag=1, tile_m=128, splitk=5))
    # conv8p: one 16 x 16 patch at every accepted tile_n, and a 2 x 1 patch grid at B = 2
    c8 = dict(ks=3, tile_m=256, stages=8)
    for N in (72, 136, 160):
        for tn in (64, 96, 128, 160, 192):
            rows.append(case(f"conv8p_1patch_N{N}_tn{tn}", "conv8p", 1, 16, 16, 64, N, **c8, tile_n=tn, ld_extra=(8, 24)[(N + tn) // 8 % 2]))
    for N, tn in ((72, 64), (136, 96), (160, 160)):
        rows.append(case(f"conv8p_2x1_B2_N{N}_tn{tn}", "conv8p", 2, 32, 16, 64, N, **c8, tile_n=tn, rowbias=True, residual=True))
    rows.append(case("conv8p_tail_split_1x512", "conv8p", 1, 16, 16, 512, 160, **c8, tile_n=160))
    rows.append(case("conv8p_tail_split_3x128_skip", "conv8p", 3, 16, 16, 128, 160, **c8, tile_n=160, skip=64, colstats=True))
    rows.append(case("subpix_1_16x16_64_64", "subpix", 1, 16, 16, 64, 64, **c8, up=1, w_sub=True))
    rows.append(case("subpix_2_16x32_128_64", "subpix", 2, 16, 32, 128, 64, **c8, up=1, w_sub=True, ld_extra=24))      # (N = 72 is refused)
    # depth-to-space store (SRGAN sub-pixel layers): out_ld = C + 8
    for (H, W, B) in ((16, 16, 2), (40, 24, 1)):
        for epi in ("none", "prelu"):
            for sk in (0, 3):
                rows.append(case(f"d2s_{H}x{W}_{epi}_s{sk}", "generic", B, H, W, 64, 256, ks=3, mode="d2s", epi=epi, splitk=sk))
    return rows


DENSE_CASES = _dense()
TRANSPOSED_CASES = _transposed()
CONV_CASES = _convs()
CASES = DENSE_CASES + TRANSPOSED_CASES + CONV_CASES
assert len({c["id"] for c in CASES}) == len(CASES)
