"""Pure-Python helpers of tests/test_gpu_gemm_f32.py (no device needed: tests/test_gemm_cases.py runs them on the CPU).

1. The launch rules of the exact-f32 GEMM (csrc/det_gemm.hip), restated.  If a launch rule changes, the restatement here changes with it
   (the GPU tests assert the v2 plan against wd_gemm_nt_workspace before every launch).

     wd_gemm_nt_f32 (v1):    gemm_nt_kernel<4,4> (128 x 128 tiles) iff ceil(M / 128) ceil(N / 128) >= 192, else gemm_nt_kernel<2,2> (64 x 64);
                             <2,2> runs as two K slices that meet through atomicAdd (bias / ReLU then in a second pass, wd_bias_relu_f32)
                             iff there is no residual, N % 4 == 0, K >= 2048 and ceil(M / 64) ceil(N / 64) < 512
     wd_gemm_nt_ws_f32 (v2): gemm_nt_v2_kernel + gemm_reduce_kernel iff M >= 256, N >= 256, K >= 1024, N % 4 == 0, K % 32 == 0 and M K, N K < 2^31
                             (otherwise it falls through to v1); the slices double while tiles * splitk < 448 and K / (2 splitk) >= 512
     both:                   K runs in slabs of 32; slice z takes slabs [z per, min((z + 1) per, nslab)), per = ceil(nslab / splitk)

2. Integer operands: position-dependent values in [-3, 3] (a wrong row, column or slab changes the answer), bias and residual in [-8, 8].
   With K <= 8192 every partial sum stays below 2^24, so every summation order, atomics included, gives the integer product bit for bit.
"""
import torch

BK = 32
V2_TARGET_WGS = 448
V1_SPLIT_TILES = 512
V1_BIG_TILES = 192
MAX_K = 8192


def cdiv(a, b):
    return (a + b - 1) // b


def slab_runs(k, splitk):
    """Slabs per slice, in slice order."""
    nslab = cdiv(k, BK)
    per = cdiv(nslab, splitk)
    return [max(min((z + 1) * per, nslab) - z * per, 0) for z in range(splitk)]


def v1_plan(m, n, k, residual=False):
    """-> (kernel '4x4' | '2x2', K slices)"""
    if cdiv(m, 128) * cdiv(n, 128) >= V1_BIG_TILES:
        return '4x4', 1
    split = not residual and n % 4 == 0 and k >= 2048 and cdiv(m, 64) * cdiv(n, 64) < V1_SPLIT_TILES
    return '2x2', 2 if split else 1


def v2_slices(m, n, k):
    """K slices of the v2 path; 0 = the shape stays on v1."""
    if m < 256 or n < 256 or k < 1024 or n % 4 or k % 32 or m * k >= 1 << 31 or n * k >= 1 << 31:
        return 0
    tiles = cdiv(m, 128) * cdiv(n, 128)
    splitk = 1
    while tiles * splitk < V2_TARGET_WGS and k // (splitk * 2) >= 512:
        splitk *= 2
    return splitk


def v2_workspace(m, n, k):
    return v2_slices(m, n, k) * m * n * 4


# (M, N, K, residual, expected v1 plan): the v1 shapes of the issue
V1_SHAPES = [
    (1, 1, 4, False, ('2x2', 1)), (63, 65, 4, False, ('2x2', 1)), (65, 63, 36, False, ('2x2', 1)), (64, 64, 32, False, ('2x2', 1)),
    (64, 64, 64, False, ('2x2', 1)), (130, 70, 96, False, ('2x2', 1)),
    (70, 130, 2048, False, ('2x2', 1)),            # N % 4 != 0: stays unsplit
    (100, 64, 2048, False, ('2x2', 2)),
    (130, 68, 2052, False, ('2x2', 2)),            # slices of 33 and 32 slabs, the last slab 4 wide
    (1984, 1024, 2052, False, ('2x2', 2)),         # 496 tiles: split
    (2048, 1024, 2052, False, ('2x2', 1)),         # 512 tiles: unsplit
    (100, 64, 2044, False, ('2x2', 1)),            # K below the limit
    (100, 64, 2048, True, ('2x2', 1)),             # a residual switches the split off
    (24449, 100, 36, False, ('4x4', 1)), (12200, 130, 68, False, ('4x4', 1)),
]
# (M, N, K, expected slices, expected slabs per slice): the v2 shapes of the issue; 0 slices = falls through to v1
V2_SHAPES = [
    (256, 256, 1024, 2, [16, 16]),
    (257, 260, 1056, 2, [17, 16]),                 # last tile: one valid row, four valid columns
    (256, 256, 2080, 4, [17, 17, 17, 14]),
    (300, 256, 8192, 16, [16] * 16),
    (3457, 2048, 1024, 1, [32]),
    (255, 256, 1024, 0, None), (256, 256, 1028, 0, None),
]
FLOAT_SHAPES = [(130, 68, 2052), (12200, 130, 68), (257, 260, 1056)]      # one per kernel: <2,2> (two atomic slices), <4,4>, v2
EPILOGUES = [(b, r, relu) for b in (False, True) for r in (False, True) for relu in (False, True)]


def operands(m, n, k, device='cpu'):
    """A (M, K), Bt (N, K) in [-3, 3], bias (N,), residual (M, N) in [-8, 8]: float32 tensors of integers, a function of the position."""
    def grid(rows, cols, salt, mod, off):
        i = torch.arange(rows, dtype=torch.int64, device=device).view(-1, 1)
        j = torch.arange(cols, dtype=torch.int64, device=device).view(1, -1)
        v = ((i + salt) * 73856093) ^ ((j + 1) * 19349663)            # an integer hash of the position
        v = ((v ^ (v >> 13)) * 83492791) & 0x7fffffff
        return (((v >> 7) % mod) - off).float()
    return grid(m, k, 1, 7, 3), grid(n, k, 100003, 7, 3), grid(1, n, 200003, 17, 8).view(-1), grid(m, n, 300007, 17, 8)


def exact_product(a, bt, bias=None, residual=None, relu=False):
    """The integer answer in float64: a float64 matmul of integers whose sums stay far below 2^53 is the int64 product."""
    out = a.double() @ bt.double().t()
    if bias is not None:
        out = out + bias.double()
    if residual is not None:
        out = out + residual.double()
    return torch.relu(out) if relu else out


def gamma(n_ops):
    """Higham's gamma_n for float32, u = 2^-24."""
    u = 2.0 ** -24
    return n_ops * u / (1 - n_ops * u)


def float_bound(a, bt, bias, residual, splitk):
    """Elementwise bound of a float32 GEMM against float64: gamma_n (|A| |B|^T + |bias| + |residual|), n = 2 K + splitk + 3 (the matrix
    instruction may round products and sums separately; splitk partial sums meet; bias, residual and the final store round once each)."""
    k = a.shape[1]
    mag = a.double().abs() @ bt.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()
    if residual is not None:
        mag = mag + residual.double().abs()
    return gamma(2 * k + splitk + 3) * mag
