"""A GEMM descriptor holds raw device pointers; ops.make_gemm_desc must keep the tensors it was given alive.  Without that, an
argument built in the call expression (`bias=interleave(cb)`) goes back to the caching allocator at once, the next allocation of
that size gets its memory, and the launch reads whatever was written there -- which made results depend on what had been
allocated and freed earlier in the process."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_descriptor_keeps_temporary_arguments_alive():
    from minddiffusion_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    M, C, N = 128, 64, 128
    x = torch.randn(M, C, generator=g).to(DEV, torch.float16)
    wp = ops.pack_gemm_weight((torch.randn(N, C, generator=g) / 8).to(DEV, torch.float16))
    bias = torch.randn(N, generator=g).to(DEV)

    def run(d):
        ws = ops.new_gemm_workspace(max(ops.gemm_workspace_bytes(d), 16), DEV)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        ops.gemm_run(d)
        torch.cuda.synchronize()

    want = torch.empty((M, N), dtype=torch.float16, device=DEV)
    run(ops.make_gemm_desc(x, wp, N, 1, M, 1, C, want, N, bias=bias, splitk=1))
    got = torch.empty((M, N), dtype=torch.float16, device=DEV)
    d = ops.make_gemm_desc(x, wp, N, 1, M, 1, C, got, N, bias=bias + 0.0, splitk=1)     # a temporary with bias's values
    junk = [torch.full((N,), 1e4, device=DEV) for _ in range(8)]       # same-size allocations: the first takes a freed block
    run(d)
    assert torch.equal(got, want), "the launch read a bias whose memory had been reused"
    del junk
