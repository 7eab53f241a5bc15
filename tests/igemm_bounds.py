"""Bounds shared by the per-op tests of the implicit GEMM (test_reduced_precision_gpu.py, test_igemm_tiles_gpu.py): one definition per bound.

16-bit storage (kpf_conv2d_h16): the kernel is the fp32-accumulated product of the operands AS STORED, so against float64 on the same rounded
operands only the output rounding remains (eps = 2^-8 bf16, 2^-11 f16, relative)."""
import torch

PREC = {"bf16": (torch.bfloat16, 2.0 ** -8), "f16": (torch.float16, 2.0 ** -11)}
NCHW_TOL = 2e-6  # the heads' fp32 NCHW output of the 16-bit path: only the accumulation order differs


def h16_excess(got, ref, eps, kind):
    """got, ref float64 of one shape -> (what is left of the error above the bound, <= 0 when it holds; the bound's name).
      "gelu": the 9-operation GELU of the 16-bit epilogues (csrc/kpf_common.h kpf_gelu_h16) is good to 2.6e-5 ABSOLUTE on top of the output
              rounding:  |got - ref| <= 1.3 * tol * |ref| + 3.5e-5,  tol = 1.01 * eps;
      "nchw": fp32 output:  max|got - ref| / max|ref| < 2.5 * NCHW_TOL + 1e-6;
      else:   elementwise relative with a floor at 1e-3 of the range:  max(|got - ref| / (|ref| + 1e-3 max|ref|)) < 2.5 * tol + 1e-6."""
    tol = 1.01 * eps
    if kind == "gelu":
        return float(((got - ref).abs() - (1.3 * tol * ref.abs() + 3.5e-5)).max()), "gelu"
    if kind == "nchw":
        return float((got - ref).abs().max() / (ref.abs().max() + 1e-12)) - (2.5 * NCHW_TOL + 1e-6), "nchw"
    return float(((got - ref).abs() / (ref.abs() + ref.abs().max() * 1e-3)).max()) - (2.5 * tol + 1e-6), "rounding"
