"""The training path's environment switches: every name, its default and what it selects, in one table.

The environment is read at every call (tests and A/B runs flip a switch between two steps); only GECCO_DW_BLOCKS is read once, at
import, by the module that uses it.  A name that is not in the table is a KeyError, not a switch that silently does nothing."""
from __future__ import annotations

import os

# name -> (default, what the values select).  Default "1": on unless set to "0".  Default "0": opt-in, on only when set to "1".
# Any other default: a valued switch, read with `value()`.
SWITCHES: dict[str, tuple[str, str]] = {
    "GECCO_DW_BLOCKS": ("768", "blocks a weight-gradient launch aims for (groups x output tiles)"),
    "GECCO_WEIGHT_IMAGES": ("1", "0: weight images per linear call instead of per step in batched launches"),
    "GECCO_LOOKUP_BWD": ("sorted", "atomic: the pyramid gradient by float atomics instead of sort + gather"),
    "GECCO_TRAIN_AMP": ("1", "0: split-bf16 linears under torch.autocast(float16) too"),
    "GECCO_TRAIN_DOTSTATS": ("1", "0: the AdaGN backward's column statistics from a pass of their own, not the dX product's epilogue"),
    "GECCO_TRAIN_DOTRES": ("1", "0: in an fp16-tensor layer those statistics from a separate pass after the second dX product"),
    "GECCO_TRAIN_DW_STREAM": ("1", "0: weight gradients on the main stream"),
    "GECCO_TRAIN_DW_STREAM_CAPTURE": ("0", "1: the side-stream fork / join also inside a hipGraph capture"),
    "GECCO_TRAIN_DW_REDUCE": ("launch", "kernel: the group partials of an fp16 weight gradient summed inside its launch"),
    "GECCO_TRAIN_ADAGNPRO": ("1", "0: AdaGN materialised instead of applied as a GEMM prologue"),
    "GECCO_TRAIN_IO16": ("1", "0: fp32 tensors for K | V, q, the attention output and their gradients under autocast(float16)"),
    "GECCO_TRAIN_ATTN16": ("1", "0: split-bf16 attention under autocast(float16) too"),
    "GECCO_TRAIN_ATTN": ("fused", "gemm: attention with materialised scores on the strided-batched GEMM"),
    "GECCO_TRAIN_DU16": ("1", "0: the MLP backward's du as an fp32 tensor"),
    "GECCO_TRAIN_ACTBWD": ("1", "0: the activation backward as a kernel of its own, not the dX product's epilogue"),
    "GECCO_TRAIN_ACTKEEP": ("1", "0: the activation forward as a kernel of its own, not the first GEMM's epilogue"),
    "GECCO_TRAIN_A16": ("1", "0: the LDS-DMA GEMM instead of the A-stationary fp16 kernels"),
    "GECCO_TRAIN_H8FWD": ("1", "0: the split-bf16 step's AdaGN-prologue forward products on the LDS-DMA GEMM, not the h8 kernel"),
    "GECCO_TRAIN_H16": ("1", "0: an MLP's hidden layer as an fp32 tensor under autocast(float16)"),
    "GECCO_TRAIN_Y16": ("0", "1: fp16(AdaGN(x)) kept by the forward, both weight-gradient operands as fp16 images"),
    "GECCO_TRAIN_CNBLOCK": ("1", "0: a CNBlock as several autograd Functions"),
    "GECCO_TRAIN_INPROJ_SIDE": ("1", "0: the packed in_proj gradient joined on the main stream"),
    "GECCO_TRAIN_INPROJ_SPLIT": ("1", "0: plain slices of the packed in_proj weight (autograd's slice backward)"),
}


def value(name: str) -> str:
    """The switch's value now: the environment's, else the table's default."""
    return os.environ.get(name, SWITCHES[name][0])


def enabled(name: str) -> bool:
    """A default-on switch is off only for "0"; an opt-in switch (default "0") is on only for "1"."""
    default = SWITCHES[name][0]
    v = os.environ.get(name, default)
    return v == "1" if default == "0" else v != "0"
