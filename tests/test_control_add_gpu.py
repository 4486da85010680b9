"""mdx_control_add_f16 on the GPU (ops.ControlAdd): dst[s][r] = fp16_rne(fmaf(scale[s][r], src[s][src_row[r]], dst[s][r])) in
place, for several segments in one launch, the row map and the scales read from device tables when the kernel runs.

The reference is the torch fp32 restatement (dst.float() + s * src.float()).half().  With dyadic scales the product is exact in
fp32, so the fused and the unfused sum agree bit for bit and torch.equal is required; a non-dyadic scale differs from the
unfused form by at most the product's fp32 rounding, i.e. at most 1 fp16 ulp after the final rounding."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NB = 3
EPR = (4096, 2048, 512, 8, 4104)            # elements per row: whole blocks, one chunk, and a row that ends mid-block
SCALES = (0.5, 0.75, 1.0, 1.5, 2.0)         # dyadic: scale * src is exact
ROWS = (-1, 0, 1)                           # row 0 is not touched; rows 1, 2 read source rows 0, 1
GUARD = 64                                  # halves on either side of every dst


def _case(seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    bufs, dsts, srcs = [], [], []
    for e in EPR:
        buf = (torch.randn(NB * e + 2 * GUARD, generator=g) * 2).to(torch.float16).to(DEV)
        bufs.append(buf)
        dsts.append(buf[GUARD:GUARD + NB * e].view(NB, e))
        srcs.append((torch.randn(2, e, generator=g) * 2).to(torch.float16).to(DEV))
    return bufs, dsts, srcs


def _expected(dsts, srcs, rows, scale):
    """scale: [n_seg][NB] python floats."""
    out = []
    for s, (d, x) in enumerate(zip(dsts, srcs)):
        e = d.clone()
        for r, q in enumerate(rows):
            if q >= 0:
                e[r] = (d[r].float() + scale[s][r] * x[q].float()).half()
        out.append(e)
    return out


def _ordered(h):
    """fp16 bit patterns as integers that are monotone in the value: neighbours differ by 1."""
    v = h.view(torch.int16).to(torch.int32)
    return torch.where(v < 0, -(v & 0x7fff), v)


def test_five_segments_one_launch_bit_exact_with_untouched_row_and_guards():
    from minddiffusion_amd import ops
    bufs, dsts, srcs = _case()
    before = [b.clone() for b in bufs]
    scale = [[s] * NB for s in SCALES]
    want = _expected(dsts, srcs, ROWS, scale)
    ops.control_add(dsts, srcs, ROWS, torch.tensor(scale))
    torch.cuda.synchronize()
    for s, e in enumerate(EPR):
        assert torch.equal(dsts[s], want[s]), f"segment {s}"
        assert torch.equal(dsts[s][0], before[s][GUARD:GUARD + e]), f"segment {s}: row 0 (src_row -1) changed"
        assert not torch.equal(dsts[s][1], before[s][GUARD + e:GUARD + 2 * e])
        assert torch.equal(bufs[s][:GUARD], before[s][:GUARD]) and torch.equal(bufs[s][-GUARD:], before[s][-GUARD:]), \
            f"segment {s}: guard band changed"


def test_per_row_scales_and_a_non_dyadic_scale_within_one_ulp():
    from minddiffusion_amd import ops
    _, dsts, srcs = _case(seed=6)
    scale = [[0.0, 0.37, 0.37 * (s + 1)] for s in range(len(EPR))]
    want = _expected(dsts, srcs, (1, 0, 1), scale)
    ops.control_add(dsts, srcs, (1, 0, 1), torch.tensor(scale))
    torch.cuda.synchronize()
    for s in range(len(EPR)):
        assert torch.equal(dsts[s][0], want[s][0])          # scale 0: the row is rewritten with its own bits
        ulps = (_ordered(dsts[s]) - _ordered(want[s])).abs().max().item()
        assert ulps <= 1, f"segment {s}: {ulps} ulp"


def test_changing_the_tables_changes_the_result_with_the_same_descriptor():
    from minddiffusion_amd import ops
    _, dsts, srcs = _case(seed=7)
    ca = ops.ControlAdd(dsts)
    base = [d.clone() for d in dsts]
    ca.run()                                        # no row map yet: every row is -1 and nothing changes
    torch.cuda.synchronize()
    assert all(torch.equal(d, b) for d, b in zip(dsts, base))
    ca.set_sources(srcs)
    desc_addr, ptr_table = id(ca.desc), ca.src_ptrs.data_ptr()
    for rows, sc in (((0, 1, -1), 1.0), ((1, 1, 0), 0.5), ((-1, -1, -1), 2.0)):
        scale = [[sc] * NB for _ in EPR]
        want = _expected(dsts, srcs, rows, scale)
        ca.set_rows(rows)
        ca.set_scale(sc)
        ca.run()
        torch.cuda.synchronize()
        assert all(torch.equal(d, w) for d, w in zip(dsts, want)), (rows, sc)
    # other source buffers: the pointer table is rewritten, the descriptor is not
    srcs2 = [x.clone() * 0.5 for x in srcs]
    ca.set_sources(srcs2)
    ca.set_rows((0, 0, 1))
    ca.set_scale(1.0)
    want = _expected(dsts, srcs2, (0, 0, 1), [[1.0] * NB for _ in EPR])
    ca.run()
    torch.cuda.synchronize()
    assert all(torch.equal(d, w) for d, w in zip(dsts, want))
    assert id(ca.desc) == desc_addr and ca.src_ptrs.data_ptr() == ptr_table and ca.table_writes == 2


def test_python_side_refusals():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    _, dsts, srcs = _case(seed=8)
    ca = ops.ControlAdd(dsts)
    with pytest.raises(MdxError, match="16-byte aligned"):
        ca.set_sources([x if s else torch.zeros(2 * EPR[0] + 8, dtype=torch.float16, device=DEV)[4:4 + 2 * EPR[0]].view(2, -1)
                        for s, x in enumerate(srcs)])
    with pytest.raises(MdxError, match="does not match"):
        ca.set_sources(srcs[::-1])
    ca.set_sources(srcs)
    with pytest.raises(MdxError, match="row map"):
        ca.set_rows((0, 1, 2))                      # the sources have two rows
    with pytest.raises(MdxError, match="row map"):
        ca.set_rows((0, 1))
    with pytest.raises(MdxError, match="segments"):
        ops.ControlAdd([dsts[0]] * 17)


def test_a_launch_larger_than_one_grid_pass():
    """2048 blocks x 256 threads x 4 chunks cover 16 Mi halves a pass: a larger segment takes the grid-stride loop."""
    from minddiffusion_amd import ops
    e = 2048 * 256 * 4 * 8 // 2 + 8 * 1000      # per row; two rows: one pass and a part of the second
    g = torch.Generator(device=DEV).manual_seed(9)
    dst = torch.randn(2, e, generator=g, device=DEV).to(torch.float16)
    src = torch.randn(2, e, generator=g, device=DEV).to(torch.float16)
    want = (dst.float() + 1.5 * src.flip(0).float()).half()
    ops.control_add([dst], [src], (1, 0), 1.5)
    torch.cuda.synchronize()
    assert torch.equal(dst, want)
