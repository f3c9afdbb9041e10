"""The weight-streaming MFMA GEMM for 9..64 rows (csrc/gemm_rows.hip, ops.gemm_nt_rows / gemm_nt_rows_glu): float64 references at every row-tile count and
ragged column count, exact small-integer products (a swapped row / column map, a wrong k order inside a fragment and a dropped K slice all change them),
untouched rows and columns past the result, launch-to-launch bits, the GLU form against its two-step definition, and the domain through the raw ABI."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS_ALL = [9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
SMALL = [(256, 128, 256), (36, 128, 36), (300, 128, 384)]                                   # N, K, ldc
LARGE = [(1000, 2048, 1000), (4099, 2048, 4099), (2048, 8192, 2048), (64, 8192, 64), (132, 8256, 132), (33000, 2048, 33008)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from ecg_byte_amd import decoder_ops
    return decoder_ops


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=2)
def _weights(N, K):
    """B, B2 and their float64 copies: drawn once per shape, shared by every row count, never written."""
    b, b2 = _bf(N, K, scale=K ** -0.5, seed=222), _bf(N, 64, scale=0.1, seed=224)
    return b, b2, b.double(), b2.double()


def _close(got, ref, atol=2e-2, rtol=2 ** -7):
    err = (got.double() - ref).abs()
    tol = atol + rtol * ref.abs()
    assert bool((err <= tol).all()), f"max err {err.max().item():.4g} (tol {tol.flatten()[err.argmax()].item():.4g})"


def _against_float64(ops, M, N, K, ldc, K2, a_view=False):
    b, b2, b64, b2_64 = _weights(N, K)
    if a_view:
        a = _bf(M, K + 128, seed=221)[:, 64:64 + K]                  # a column slice: lda = K + 128
        assert a.stride(0) > K
    else:
        a = _bf(M, K, seed=221)
    a2 = _bf(M, 64, seed=223) if K2 else None
    want = a.double() @ b64.T
    if K2:
        want = want + a2.double() @ b2_64.T
    for alpha in (1.0, 0.5):
        out = torch.full((64, ldc), 7.0, dtype=torch.bfloat16, device="cuda")
        got = ops.gemm_nt_rows(a, b, a2=a2, b2=b2 if K2 else None, alpha=alpha, out=out)
        assert got is out
        _close(out[:M, :N], alpha * want)
        assert bool((out[M:] == 7.0).all()) and bool((out[:, N:] == 7.0).all())


@pytest.mark.parametrize("K2", [0, 64])
@pytest.mark.parametrize("N,K,ldc", SMALL)
@pytest.mark.parametrize("M", ROWS_ALL)
def test_gemm_nt_rows_against_float64_small(ops, M, N, K, ldc, K2):
    """Every row-tile count and its edges (9..64) at one and two K steps, whole / partial / ragged column blocks, ldc > N."""
    _against_float64(ops, M, N, K, ldc, K2)


@pytest.mark.parametrize("K2", [0, 64])
@pytest.mark.parametrize("N,K,ldc", LARGE)
@pytest.mark.parametrize("M", [9, 33, 64])
def test_gemm_nt_rows_against_float64_large(ops, M, N, K, ldc, K2):
    """Sliced and unsliced K, a ragged last chunk (K 8256), one column block (N 64), many (N 33 000: K whole, direct store)."""
    _against_float64(ops, M, N, K, ldc, K2)


def test_gemm_nt_rows_takes_a_column_slice_of_a(ops):
    _against_float64(ops, 33, 1000, 2048, 1000, 64, a_view=True)


@pytest.mark.parametrize("N", [20, 300])
@pytest.mark.parametrize("M", [9, 17, 64])
def test_gemm_nt_rows_exact_integers(ops, M, N):
    """A[i][k] = ((3 i + 5 k) % 5) - 2, B[j][k] = ((7 j + k) % 3) - 1, K = 128: every product and sum is exact in fp32 and in bf16."""
    K = 128
    i, j, k = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    a = ((3 * i + 5 * k) % 5 - 2).to(torch.float32)
    b = ((7 * j + k) % 3 - 1).to(torch.float32)
    want = a @ b.T
    assert float(want.abs().max()) <= 256                                # integers a bf16 holds exactly
    got = ops.gemm_nt_rows(a.to(torch.bfloat16).cuda(), b.to(torch.bfloat16).cuda())
    assert torch.equal(got.float().cpu(), want)


@pytest.mark.parametrize("M,N,K,ldc", [(9, 36, 128, 48), (33, 300, 128, 384), (50, 1000, 2048, 1003), (64, 33000, 2048, 33008)])
def test_gemm_nt_rows_leaves_rows_and_columns_past_the_result(ops, M, N, K, ldc):
    a, b = _bf(M, K, seed=231), _bf(N, K, scale=K ** -0.5, seed=232)
    out = torch.full((64, ldc), -3.0, dtype=torch.bfloat16, device="cuda")
    ops.gemm_nt_rows(a, b, out=out)
    assert bool((out[M:] == -3.0).all()) and bool((out[:, N:] == -3.0).all())
    _close(out[:M, :N], a.double() @ b.double().T)


@pytest.mark.parametrize("M,N,K,K2", [(33, 2048, 2048, 64), (64, 4099, 2048, 0), (17, 64, 8192, 64)])
def test_gemm_nt_rows_same_bits_on_every_launch(ops, M, N, K, K2):
    a, b = _bf(M, K, seed=241), _bf(N, K, scale=K ** -0.5, seed=242)
    a2, b2 = (_bf(M, K2, seed=243), _bf(N, K2, scale=0.1, seed=244)) if K2 else (None, None)
    first = ops.gemm_nt_rows(a, b, a2=a2, b2=b2)
    torch.empty(64 << 20, device="cuda", dtype=torch.uint8).random_()
    assert torch.equal(ops.gemm_nt_rows(a, b, a2=a2, b2=b2), first)


@pytest.mark.parametrize("K2", [0, 64])
@pytest.mark.parametrize("gelu_tanh", [False, True])
@pytest.mark.parametrize("inter", [128, 1000, 8192])
@pytest.mark.parametrize("M", [9, 33, 64])
def test_gemm_nt_rows_glu_is_the_plain_form_then_glu_fwd(ops, M, inter, gelu_tanh, K2):
    K = 2048
    a, b = _bf(M, K, seed=251), _bf(2 * inter, K, scale=K ** -0.5, seed=252)
    a2, b2 = (_bf(M, K2, seed=253), _bf(2 * inter, K2, scale=0.1, seed=254)) if K2 else (None, None)
    want = ops.glu_fwd(ops.gemm_nt_rows(a, b, a2=a2, b2=b2), gelu_tanh=gelu_tanh)
    got = ops.gemm_nt_rows_glu(a, b, gelu_tanh=gelu_tanh, a2=a2, b2=b2)
    assert got.shape == (M, inter) and torch.equal(got, want)


def test_gemm_nt_rows_domain_through_the_raw_abi(ops):
    from ecg_byte_amd import _lib
    L = _lib.lib()
    a, b = _bf(65, 256 + 8, seed=261), _bf(64, 256 + 8, seed=262)
    c = torch.zeros((65, 64), dtype=torch.bfloat16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = ops._L().ecgb_gemm_nt_rows_scratch_bytes(64, 64, 256)
    buf = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def call(M, K, a_ptr=a.data_ptr(), b_ptr=b.data_ptr(), c_ptr=c.data_ptr()):
        p = lambda x: C.c_void_p(x) if x else None
        return L.ecgb_gemm_nt_rows_bf16(p(a_ptr), a.stride(0), p(b_ptr), b.stride(0), None, 0, None, 0, 0, p(c_ptr), c.stride(0), M, 64, K, 1.0,
                                        C.c_void_p(buf.data_ptr()), buf.numel(), st)

    UNSUPPORTED, INVALID = -3, -1
    assert call(64, 256) == 0
    for M in (8, 65):
        assert call(M, 256) == UNSUPPORTED and not ops.gemm_nt_rows_ok(M, 64, 256)
    assert call(32, 96) == UNSUPPORTED and not ops.gemm_nt_rows_ok(32, 64, 96)
    assert call(32, 256, a_ptr=a.data_ptr() + 8) == UNSUPPORTED
    assert not ops.gemm_nt_rows_ok(32, 64, 256, ptrs=(a.data_ptr() + 8, b.data_ptr()))
    assert ops.gemm_nt_rows_ok(32, 64, 256, strides=(a.stride(0), b.stride(0)), ptrs=(a.data_ptr(), b.data_ptr()))
    assert ops.gemm_nt_rows_ok(9, 1, 64) and ops.gemm_nt_rows_ok(64, 132096, 2048, 64) and not ops.gemm_nt_rows_ok(32, 64, 256, 32)
    assert call(32, 256, a_ptr=0) == INVALID and call(32, 256, b_ptr=0) == INVALID and call(32, 256, c_ptr=0) == INVALID
    assert b"" != (L.ecgb_last_error() or b"")
    torch.cuda.synchronize()
    assert bool((c[64:] == 0).all())
