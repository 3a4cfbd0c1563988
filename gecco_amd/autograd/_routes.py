"""Which kernel takes this product: every route predicate of the training path.  The Functions ask here; nothing here launches."""
from __future__ import annotations

from .. import _lib, hip_ops
from ._base import _lin_precision, _train_precision
from ._switches import enabled, value


def _resolve(prec: str | None, rows: int, K: int, Nout: int) -> str:
    """The arithmetic of ONE product: `prec` (None: the training precision), except that an "fp16" request for a shape the fp16
    LDS-DMA kernel does not take goes back to the training precision (hip_ops.linear would run it on the exact-fp32 kernel)."""
    if prec is None:
        return _train_precision()
    if prec == "fp16" and not _lib.load().gecco_linear_image_ok_f16(rows, K, Nout, 0):
        return _train_precision()
    return prec


def _image_ok(rows: int, K: int, Nout: int, prec: str = "bf16x3") -> bool:
    lib = _lib.load()
    return bool(lib.gecco_linear_image_ok_f16(rows, K, Nout, 0) if prec == "fp16" else lib.gecco_linear_image_ok(rows, K, Nout, 0))


def _pro_ok(R: int, K: int, Nout: int) -> bool:
    """The AdaGN-as-prologue Functions: split-bf16 training precision, shapes the LDS-DMA kernels take with a prologue."""
    prec = _lin_precision()
    if not enabled("GECCO_TRAIN_ADAGNPRO") or prec not in ("bf16x3", "fp16") or K > 1024 or R % 32:
        return False
    lib = _lib.load()
    return bool(lib.gecco_linear_image_ok_f16(R, K, Nout, 1) if prec == "fp16" else lib.gecco_linear_image_ok(R, K, Nout, 1))


def _io16_ok(R: int, Cc: int, H: int, I: int) -> bool:
    """Under the autocast(float16) arithmetic the projections K | V and q of a layer, the unpool attention's output and their gradients
    are read only by kernels that round them to fp16 on the way in (both attentions and their backward, out_proj and its dX / dW products,
    the dX / dW products of kv_proj | q_proj): they are then fp16 TENSORS, as in the reference's autocast run (Lightning's
    precision="16-mixed": nn.Linear / SDPA outputs are halves there, example_configs/shapenet_airplane_unconditional.py:74) — the same
    operand bits, half the bytes of fifteen crossings of HBM per layer (~1.7 GB at the shipped batch).  Shapes every kernel of that
    chain takes: whole 128-row blocks, 64 inducers, head dims 16 / 32 / 48 / 64, feature_dim 128 / 256 / 384 / 512.  GECCO_TRAIN_IO16=0: fp32 tensors."""
    if not enabled("GECCO_TRAIN_IO16") or _lin_precision() != "fp16" or not enabled("GECCO_TRAIN_ATTN16"):
        return False
    hd = Cc // H
    return (I == 64 and Cc % H == 0 and hd in (16, 32, 48, 64) and Cc in (128, 256, 384, 512) and R >= 128 and R % 128 == 0
            and _fused_attn_ok(I, hd) and _a16_ok("fp16", R, Cc, 3 * Cc) and _image_ok(R, Cc, Cc, "fp16") and _image_ok(R, 2 * Cc, Cc, "fp16"))


def _du16_ok(prec: str, R: int, Nout: int, K: int, K0: int) -> bool:
    """Under the autocast(float16) arithmetic the gradient du = (dy W2) act'(u) of an MLP's hidden pre-activation is read again only by
    the matrix pipe — the first linear's weight gradient and its dX product — as an fp16 operand either way (the reference's autocast
    backward holds it as an fp16 tensor: autograd of models/mlp.py:5-39 under precision="16-mixed"): the dX product's epilogue stores it
    as halves, half the bytes of its three crossings of HBM, and the dX product that reads it runs on fp16 tiles (2 x fewer bytes into
    the CU per FLOP).  Same operand bits as rounding the fp32 tensor at the consumers; the bias gradient (column sums of du) is then formed
    from the halves.  (R, Nout -> K): the product that forms du; K0: the first linear's input width.  GECCO_TRAIN_DU16=0: fp32 du."""
    if (prec != "fp16" or not enabled("GECCO_TRAIN_DU16") or not enabled("GECCO_TRAIN_ACTBWD")
            or not enabled("GECCO_TRAIN_DOTSTATS") or not _a16_ok(prec, R, Nout, K)):
        return False
    lib = _lib.load()
    return bool(K % 32 == 0 and R >= 128 and R % 32 == 0 and K0 % 4 == 0 and lib.gecco_linear_actbwd_ok(R, Nout, K, 2)
                and lib.gecco_linear_actbwd_ok(R, K, K0, 2))


def _a16_ok(prec: str, R: int, K: int, Nout: int) -> bool:
    """The A-stationary fp16 kernels (gecco_linear_astat16_*) take this product: the autocast(float16) arithmetic, whole 128-row blocks,
    an operand of <= 512 columns held in registers, 64-column output tiles.  GECCO_TRAIN_A16=0: the LDS-DMA GEMM instead."""
    return (prec == "fp16" and enabled("GECCO_TRAIN_A16")
            and bool(_lib.load().gecco_linear_astat16_ok(R, K, Nout)))


def _h8_ok(prec: str, R: int, K: int, Nout: int) -> bool:
    """The split-bf16 training FORWARD's AdaGN-prologue products on the h8 A-stationary kernel (gecco_linear_h8_train_f32): the same
    accuracy class as split-bf16 (fp16 main product + two fp8 cross terms), the operand rows in registers and the weight stream read
    once per 128 rows.  Forward only: activations and weights fit the fp16 / fp8 operand ranges, unscaled gradients do not, so the
    backward products keep split-bf16.  Only where the model's arithmetic is one of the modes that compute these very products that way
    in inference ("mixed", "w2"; "fp16"): an explicit "bf16x3" keeps true split-bf16 (fp32 exponent range, no operand clamps) in the
    forward too.  GECCO_TRAIN_H8FWD=0: the LDS-DMA split-bf16 GEMM everywhere."""
    return (prec == "bf16x3" and hip_ops.default_precision() in ("mixed", "w2", "fp16") and enabled("GECCO_TRAIN_H8FWD")
            and bool(_lib.load().gecco_linear_h8_train_ok(R, K, Nout)))


def _h16_ok(prec: str, R: int, K0: int, N0: int, Nout2: int, pro: bool) -> bool:
    """Under the autocast(float16) arithmetic the hidden layer h = act(u) of an MLP is read again only by the matrix pipe — the
    second linear's forward and its weight gradient — as an fp16 operand either way (the reference's autocast stores it as fp16
    too): the first GEMM's epilogue stores it as fp16 (`gecco_linear_act_keep_h16`), half the bytes of its three crossings of HBM.
    u (the pre-activation the backward differentiates) stays fp32."""
    if prec != "fp16" or not enabled("GECCO_TRAIN_H16") or R < 128 or R % 32 or N0 % 8 or Nout2 % 4:
        return False
    lib = _lib.load()
    return bool(lib.gecco_linear_image_ok_f16(R, K0, N0, int(pro)) and lib.gecco_linear_image_ok_f16(R, N0, Nout2, 0))


def _y16_ok(R: int, K: int, Nout: int) -> bool:
    """The weight gradient dY^T X of a linear whose dY is an fp16 tensor (`_io16_ok`, `_du16_ok`) on fp16 images of BOTH operands: the
    forward kernel stores the operand it forms, y16 = fp16(AdaGN(x)), and the weight-gradient kernel takes its slabs global -> LDS by DMA
    (gemm_tn_f16_dma_kernel: whole 128 x 128 tiles).  Default off: X = x with the AdaGN apply while it is staged."""
    # OPT-IN (measured and lost, profiles/r06_negative_results.txt item 10): the kernel alone 168 -> 143 us, the step 16.77 -> 17.26 ms
    return enabled("GECCO_TRAIN_Y16") and R % 32 == 0 and K % 128 == 0 and Nout % 128 == 0


def _attn_pr() -> int:
    """Arithmetic code of the fused attention kernels (forward and the backward that recomputes P with the same operands): the
    training precision, or — under autocast(float16), where torch runs scaled_dot_product_attention / nn.MultiheadAttention and their
    backward with fp16 operands — 2: one fp16 plane per operand, one MFMA per product (GECCO_TRAIN_ATTN16=0: split-bf16 there too)."""
    if _lin_precision() == "fp16" and enabled("GECCO_TRAIN_ATTN16"):
        return 2
    return min(hip_ops.PRECISIONS[_train_precision()], 1)


def _fused_attn_ok(I: int, hd: int) -> bool:
    """Shapes the fused attention kernels take (every shipped config: 64 inducers, head dim d / 8); others run the
    strided-batched GEMM form below."""
    return I == 64 and hd % 8 == 0 and 8 <= hd <= 64 and value("GECCO_TRAIN_ATTN") != "gemm"
