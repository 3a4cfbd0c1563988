"""fp64 restatement of the fixed-sweep Sinkhorn iteration of gecco_sinkhorn_f32 / oracle/cpu_ref.py::sinkhorn_cost that also returns the
potentials and the plan, and the gradient of <P, C> with the plan held constant by torch autograd — the references of
tests/test_hip_sinkhorn.py.  Not a test module."""
import math

import torch


def solve(a, b, epsilon, iterations):
    """a (B, N, 3), b (B, M, 3) -> value (B,), f (B, N), g (B, M), P (B, N, M), all fp64; the cost is cpu_ref.distance_matrix's formula."""
    a, b = a.detach().double(), b.detach().double()
    N, M = a.shape[1], b.shape[1]
    Cm = ((a * a).sum(-1)[:, :, None] + (b * b).sum(-1)[:, None, :] - 2 * a @ b.transpose(1, 2)).clamp_min(0.0)
    f = torch.zeros(a.shape[0], N, dtype=torch.float64)
    g = torch.zeros(a.shape[0], M, dtype=torch.float64)
    for _ in range(iterations):
        f = -epsilon * torch.logsumexp((g[:, None, :] - Cm) / epsilon - math.log(M), dim=2)
        g = -epsilon * torch.logsumexp((f[:, :, None] - Cm) / epsilon - math.log(N), dim=1)
    P = torch.exp((f[:, :, None] + g[:, None, :] - Cm) / epsilon - math.log(N) - math.log(M))
    return (P * Cm).sum((1, 2)), f, g, P


def plan_gradient(a, b, epsilon, iterations, rows=512):
    """d/da, d/db of (P.detach() * C_diff).sum() by autograd in fp64, C_diff = |a_i - b_j|^2 from coordinate differences, P the plan of
    `solve`.  The sum is taken over blocks of `rows` rows of a (the gradients accumulate), so that the (N, M, 3) differences of a large pair
    never exist at once."""
    value, f, g, P = solve(a, b, epsilon, iterations)
    a = a.detach().double().requires_grad_(True)
    b = b.detach().double().requires_grad_(True)
    for r0 in range(0, a.shape[1], rows):
        diff = a[:, r0:r0 + rows, None, :] - b[:, None, :, :]
        (P[:, r0:r0 + rows] * (diff * diff).sum(-1)).sum().backward()
    return value, a.grad, b.grad
