"""The checkers of tests/adam_ref.py reject what they must.  An fp32 restatement of adam.hip on the CPU, written in the
kernel's order of operations, stands in for the kernel: unchanged it passes every checker on the inputs of the GPU cases
D3, F1 (M = 4) and C1; with one defect built in, the checker that owns that defect fails."""
import math

import pytest
import torch

import adam_ref as A

F32 = torch.float32


def adam32(p, g, m, v, lr, t, betas, eps, defect=None):
    """adam_one of adam.hip in fp32 torch: m + (g - m)(1 - b1), v b2 + (1 - b2) g g, p - step_size (m / denom)."""
    b1, b2 = betas
    omb1, omb2, b2f = (torch.tensor(x, dtype=F32) for x in (1.0 - b1, 1.0 - b2, b2))
    if defect == "omb2 in fp32":
        omb2 = torch.tensor(1.0, dtype=F32) - b2f
    ss = torch.tensor(lr / (1.0 - b1 ** t), dtype=F32)
    ib = torch.tensor(1.0 / math.sqrt(1.0 - b2 ** (t + 1 if defect == "t off by one" else t)), dtype=F32)
    m1 = m + (g - m) * omb1
    v1 = v * b2f + omb2 * g * g
    if defect == "eps in sqrt":
        denom = torch.sqrt(v1 + torch.tensor(eps, dtype=F32)) * ib
    else:
        denom = torch.sqrt(v1) * ib + torch.tensor(eps, dtype=F32)
    p1 = p - ss * (m1 / denom)
    if defect == "tail":
        keep = p.numel() - p.numel() % 4
        flat = lambda new, old: torch.cat([new.reshape(-1)[:keep], old.reshape(-1)[keep:]]).view(old.shape)
        p1, m1, v1 = flat(p1, p), flat(m1, m), flat(v1, v)
    return p1, m1, v1


def check_d3(defect=None):
    for c in A.d3_cases():
        new = adam32(c.p, c.g, c.m, c.v, c.lr, c.t, c.betas, c.eps, defect)
        A.check_dense((c.p, c.m, c.v), new, c.g, c.lr, c.t, c.betas, c.eps, what=c.name)


def factored32(c, defect=None, first=0, count=None):
    """adam_sh_factored_kernel in fp32 torch on the Gaussians [first, first + count) -> (p, m, v), each [N,M,3]."""
    count = c.N - first if count is None else count
    g = A.factored_grad(c.xyz, c.records, c.views, c.stride, c.stride, c.deg, c.M, c.grad_scale, dtype=F32)
    if defect == "row crossing":          # the last element of a tile row takes the gradient of the next element
        row_f = 3 * (c.M - 1)
        flat = g[:, 1:].reshape(-1).clone()
        e = torch.arange(flat.numel() - 1)
        e = e[e % row_f == row_f - 1]
        flat[e] = g[:, 1:].reshape(-1)[e + 1]
        g = torch.cat([g[:, :1], flat.view(c.N, c.M - 1, 3)], dim=1)
    dc = adam32(c.p[:, :1], g[:, :1], c.m[:, :1], c.v[:, :1], c.lr_dc, c.t, c.betas, c.eps)
    rest = adam32(c.p[:, 1:], g[:, 1:], c.m[:, 1:], c.v[:, 1:], c.lr_rest, c.t, c.betas, c.eps)
    p1, m1, v1 = (torch.cat([a, b], dim=1) for a, b in zip(dc, rest))
    if defect == "dc v not decayed":
        unseen = (g[:, 0] == 0).all(dim=1)
        v1[unseen, 0] = c.v[unseen, 0]
    stop = first + count + (1 if defect == "neighbour row" else 0)
    out = []
    for new, old in ((p1, c.p), (m1, c.m), (v1, c.v)):
        x = old.clone()
        x[first:stop] = new[first:stop]
        out.append(x)
    return tuple(out)


def check_factored_range(c, new, first=0, count=None):
    count = c.N - first if count is None else count
    old = (c.p, c.m, c.v)
    A.check_factored(c, old, new, slice(first, first + count), what=c.name)
    for name, x0, x1 in zip("pmv", old, new):
        A.check_untouched(x0[:first], x1[:first], f"{c.name}: {name} below the range")
        A.check_untouched(x0[first + count:], x1[first + count:], f"{c.name}: {name} above the range")


def cache32(c, sh_new, defect=None):
    col = A.colour_cache(c.p if defect == "old coefficients" else sh_new, c.xyz_next, c.campos_next, c.deg_next, dtype=F32)
    if defect == "clamp on <= 0":
        col.bits = ((col.t <= 0).to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(dim=1).to(torch.int32)
    return A.pack_cache(col)


def check_c1(c, defect=None):
    new = factored32(c)
    check_factored_range(c, new)
    A.check_cache(cache32(c, new[0], defect), new[0], c.xyz_next, c.campos_next, c.deg_next, exact_rows=c.exact_rows,
                  before=A.sentinel(13 * c.N), what=c.name)


def test_restatement_passes_d3():
    check_d3()


@pytest.mark.parametrize("N", A.F1_SIZES[4])
def test_restatement_passes_f1_m4(N):
    for c in A.f1_cases(4, N):
        check_factored_range(c, factored32(c))


@pytest.mark.parametrize("M", list(A.F1_SIZES))
def test_restatement_passes_c1(M):
    for N in A.C1_SIZES:
        for c in A.c1_cases(M, N):
            check_c1(c)


def test_restatement_passes_a_range_and_its_cache():
    c = A.c2_case(4)
    new = factored32(c, first=c.first, count=c.count)
    check_factored_range(c, new, c.first, c.count)
    col = A.colour_cache(new[0], c.xyz_next, c.campos_next, c.deg_next, dtype=F32)
    cache = A.pack_cache(col, first=c.first, count=c.count)
    A.check_cache(cache, new[0], c.xyz_next, c.campos_next, c.deg_next, c.first, c.count, before=A.sentinel(13 * c.N),
                  exact_rows=c.exact_rows)
    with pytest.raises(AssertionError, match="above the range"):          # a cache row too many
        A.check_cache(A.pack_cache(col, first=c.first, count=c.count + 1), new[0], c.xyz_next, c.campos_next, c.deg_next,
                      c.first, c.count, before=A.sentinel(13 * c.N), exact_rows=c.exact_rows)


@pytest.mark.parametrize("defect,quantity", [("omb2 in fp32", "v is"), ("t off by one", "p is"), ("eps in sqrt", "p is"),
                                             ("tail", "m is")])
def test_dense_defects_are_rejected(defect, quantity):
    with pytest.raises(AssertionError, match=quantity):
        check_d3(defect)


def test_gradient_read_one_element_late_at_a_row_crossing_is_rejected():
    c = A.f1_cases(4, 65)[-1]
    assert c.M == 4 and c.deg == 1
    with pytest.raises(AssertionError, match="m_sh is"):
        check_factored_range(c, factored32(c, "row crossing"))


def test_undecayed_dc_moment_of_an_unseen_gaussian_is_rejected():
    c = A.f1_cases(4, 65)[-1]
    with pytest.raises(AssertionError, match="v_sh is"):
        check_factored_range(c, factored32(c, "dc v not decayed"))


def test_range_that_writes_its_neighbour_row_is_rejected():
    c = A.f2_case(4)
    check_factored_range(c, factored32(c, first=64, count=65), 64, 65)
    with pytest.raises(AssertionError, match="above the range"):
        check_factored_range(c, factored32(c, "neighbour row", first=64, count=65), 64, 65)


def test_colours_of_the_old_coefficients_are_rejected():
    c = A.c1_cases(4, 65)[0]
    with pytest.raises(AssertionError, match="rgb is"):
        check_c1(c, "old coefficients")


def test_clamp_on_less_or_equal_is_rejected():
    c = A.c1_cases(4, 65)[0]
    t = c.p[c.exact_rows[0], 0, 0] * torch.tensor(0.28209479177387814, dtype=F32) + 0.5
    assert float(t) == 0.0                                   # the case holds a colour that sits on the clamp exactly
    with pytest.raises(AssertionError, match="clamp bit 0"):
        check_c1(c, "clamp on <= 0")


def test_references_agree_with_independent_forms():
    """dense_step against torch's own float64 Adam; colour_cache's autograd Jacobian against central differences."""
    c = A.dense_case(257, 1, t=4)
    q = torch.nn.Parameter(c.p.double())
    q.grad = c.g.double()
    opt = torch.optim.Adam([q], lr=c.lr, betas=c.betas, eps=c.eps, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": c.m.double(), "exp_avg_sq": c.v.double()}
    opt.step()
    p, m, v = A.dense_step(c.p, c.g, c.m, c.v, c.lr, c.t, c.betas, c.eps)
    torch.testing.assert_close(m, opt.state[q]["exp_avg"], rtol=1e-13, atol=0)
    torch.testing.assert_close(v, opt.state[q]["exp_avg_sq"], rtol=1e-13, atol=0)
    torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-16)
    cc = A.cache_case(65, 16, 3, 3)
    col = A.colour_cache(cc.p, cc.xyz_next, cc.campos_next, 3)
    from gaussmart_amd.sh import sh_basis
    d = cc.xyz_next.double() - cc.campos_next.double()
    d = d / d.norm(dim=1, keepdim=True)
    h = 1e-6
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[j] = h
        diff = (sh_basis(3, d + e) - sh_basis(3, d - e)) / (2 * h)             # [N,16]
        Jj = (diff[:, :, None] * cc.p.double()).sum(dim=1)                      # [N,c]
        torch.testing.assert_close(col.J.view(-1, 3, 3)[:, :, j], Jj, rtol=1e-7, atol=1e-8)
