"""Argument checks of the exact EMD (metrics.emd, pairwise_set_distance(kind="emd_exact")): they raise before any launch, so they
run without a GPU; and the Python constants agree with the C header."""
import os
import re

import pytest
import torch

from gecco_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_match_header():
    src = open(os.path.join(ROOT, "include", "gecco_hip.h")).read()
    assert int(re.search(r"#define GECCO_EMD_MAX_POINTS (\d+)", src).group(1)) == metrics.EMD_MAX_POINTS
    assert int(re.search(r"#define GECCO_EMD_Q (\d+)", src).group(1)) == metrics.EMD_Q
    assert metrics.EMD_Q >= 22


def test_unequal_sizes_raise():
    with pytest.raises(ValueError, match="equal size"):
        metrics.emd(torch.zeros(2, 8, 3), torch.zeros(2, 9, 3))
    with pytest.raises(ValueError, match="equal size"):
        metrics.pairwise_set_distance(torch.zeros(2, 8, 3), torch.zeros(3, 9, 3), kind="emd_exact")


def test_too_many_points_raise():
    big = torch.zeros(1, metrics.EMD_MAX_POINTS + 1, 3)
    with pytest.raises(ValueError, match=str(metrics.EMD_MAX_POINTS)):
        metrics.emd(big, big)
    with pytest.raises(ValueError, match=str(metrics.EMD_MAX_POINTS)):
        metrics.pairwise_set_distance(big, big, kind="emd_exact")


def test_bad_arguments_raise():
    a = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="kind"):
        metrics.pairwise_set_distance(a, a, kind="emd_exactly")
    with pytest.raises(ValueError, match="l1"):
        metrics.emd(a, a, match="l3")
    with pytest.raises(ValueError, match="l1"):
        metrics.emd(a, a, average="linf")
    with pytest.raises(ValueError, match="max_rounds"):
        metrics.emd(a, a, max_rounds=0)
    with pytest.raises(ValueError):
        metrics.emd(torch.zeros(2, 8, 2), torch.zeros(2, 8, 2))


def test_cpu_tensors_have_no_fallback():
    a = torch.randn(2, 8, 3)
    with pytest.raises(_lib.GeccoHipError):
        metrics.emd(a, a)
    with pytest.raises(_lib.GeccoHipError):
        metrics.emd(a[0], a[1])
    with pytest.raises(_lib.GeccoHipError):
        metrics.pairwise_set_distance(a, a, kind="emd_exact")
