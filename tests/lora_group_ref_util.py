"""Float64 references for ONE LoRA group (halva_amd/llama.py: _LoraGroupFn, LoraGroup), stage by stage, each formed from the operands
that stage actually read - so a test can hold every element of xa's LoRA columns, y, dxa and the derived weights to the bound of
tests/gemm_ref_util.py (`held`, `delta_det`).  Nothing here calls a project kernel: the module imports without a GPU and works wherever
its tensors live (tests/test_lora_group_ref_util_cpu.py proves on the CPU that the stages compose to the peft formula and its autograd).

Notation: x [rows, K] the input (the left K columns of the operand buffer xa), W [N, K] the frozen fused weight, A_cat [G r, K] the A
factors of the G targets stacked, B_g [out_g, r], N = sum out_g, tail = ceil(G r / 8) 8 columns.

    t      = x A_cat^T                          xa[:, K : K + G r]                          n = K
    y      = [res +] xa Wc^T                    Wc = weight_cat [N, K + tail] as stored     n = K + tail
    tail   = blockdiag(scale B_g)               weight_cat[:, K:], zero elsewhere
    merged = W^T + A_cat^T tail_rows            weight_cat_t[:K], tail_rows = weight_cat_t[K : K + G r]      n = G r
    dx     merged:   dy weight_cat_t[:K]^T                                                  n = N
           unmerged: dy W + da A_cat  (with the transposed copy, or through Wc itself)      n = N, then G r
    da     = dy_g tail[rows of g, columns of g], per group block                            n = N (the GEMM contracts over all of N)

Every function returns (reference, S) in float64, S being the sum of the magnitudes of the reference's terms (what `delta_det` takes).
Leading dimensions are flattened: a [2, 100, width] operand is its [200, width] view.
"""
import torch

from gemm_ref_util import bf


def tail_width(G, r):
    return (G * r + 7) // 8 * 8


def _d(t, cols=None):
    t = t.detach().double()
    t = t.reshape(-1, t.shape[-1])
    return t if cols is None else t[:, cols[0]:cols[1]]


def _mm(a, b, *more):
    """(a b [+ ...], |a| |b| [+ ...]) for float64 a, b and further (a', b') pairs"""
    ref, S = a @ b, a.abs() @ b.abs()
    for a2, b2 in more:
        ref, S = ref + a2 @ b2, S + a2.abs() @ b2.abs()
    return ref, S


def t_ref(x, A_cat):
    """the LoRA columns of xa: x A_cat^T [rows, G r]"""
    return _mm(_d(x), _d(A_cat).t())


def y_ref(xa, Wc, res=None, cols=None):
    """[res +] xa[:, :cols] Wc[:, :cols]^T; cols = None contracts over every column of the operand buffer (padding included)"""
    c = None if cols is None else (0, cols)
    ref, S = _mm(_d(xa, c), _d(Wc, c).t())
    if res is not None:
        ref, S = ref + _d(res), S + _d(res).abs()
    return ref, S


def tail_ref(Bs, scale, r, width=None):
    """blockdiag(scale B_g) as [N, width] float64 (width defaults to the padded tail): rows of target g, columns [g r, (g + 1) r)"""
    G = len(Bs)
    width = tail_width(G, r) if width is None else width
    N = sum(B.shape[0] for B in Bs)
    out = torch.zeros(N, width, dtype=torch.float64, device=Bs[0].device)
    off = 0
    for g, B in enumerate(Bs):
        assert B.shape[1] == r
        out[off:off + B.shape[0], g * r:(g + 1) * r] = scale * _d(B)
        off += B.shape[0]
    return out


def merged_ref(W, A_cat, tail_rows):
    """what refresh_tail writes into weight_cat_t[:K]: W^T + A_cat^T tail_rows, [K, N]; tail_rows [G r, N]"""
    W, A, T = _d(W), _d(A_cat), _d(tail_rows)
    ref, S = _mm(A.t(), T)
    return W.t() + ref, W.t().abs() + S


def dx_merged_ref(dy, merged_rows):
    """dy merged_rows^T [rows, K]; merged_rows = weight_cat_t[:K] as stored"""
    return _mm(_d(dy), _d(merged_rows).t())


def dx_unmerged_ref(dy, W, da, A_cat):
    """the two products of the unmerged dgrad, each with its S: (dy W, S1, da A_cat, S2); dx = their sum.  W [N, K]: the frozen
    weight, through the transposed copy or through weight_cat's left columns - the same numbers either way."""
    r1, S1 = _mm(_d(dy), _d(W))
    r2, S2 = _mm(_d(da), _d(A_cat))
    return r1, S1, r2, S2


def two_rounding_model(r1, r2):
    """bf16(bf16(dy W) + da A): an unmerged dgrad that stores the first product in bf16 and adds the second onto it in place (the
    backward itself sums both in fp32 and rounds once; the two-rounding bound of the GPU test is written against this model)"""
    return bf(bf(r1) + r2)


def da_ref(dy, tail, outs, r):
    """[rows, G r]: block g = dy[:, rows of g] tail[rows of g, g r : (g + 1) r] - per group block, so that a stored tail with anything
    off the block diagonal shows in the kernel's result and not in the reference"""
    dy, tail = _d(dy), _d(tail)
    refs, Ss, off = [], [], 0
    for g, n in enumerate(outs):
        ref, S = _mm(dy[:, off:off + n], tail[off:off + n, g * r:(g + 1) * r])
        refs.append(ref)
        Ss.append(S)
        off += n
    return torch.cat(refs, 1), torch.cat(Ss, 1)


def wgrad_operands(dy, xa, dxa, K, outs, r, scale):
    """(left, right, factor) of every weight-gradient product of the group, in the order of the parameters - the A factors' rows, then
    each B: grad = factor * left^T right, from the operands the backward itself used (xa as the forward left it, da in dxa's columns)"""
    G = len(outs)
    dy, xa, dxa = (t.reshape(-1, t.shape[-1]) for t in (dy, xa, dxa))
    prods, off = [(dxa[:, K:K + G * r], xa[:, :K], 1.0)], 0
    for g, n in enumerate(outs):
        prods.append((dy[:, off:off + n], xa[:, K + g * r:K + (g + 1) * r], scale))
        off += n
    return prods


def wgrad_ref(left, right, factor):
    ref, S = _mm(_d(left).t(), _d(right))
    return factor * ref, factor * S


def peft_y(x, W, A_cat, Bs, scale, r, res=None):
    """the plain formula, res + x W^T + scale concat_g((x A_g^T) B_g^T), on whatever dtype its arguments have; differentiable.
    Returns (y, t) with t = x A_cat^T kept as a graph node (retain_grad gives da)."""
    t = x @ A_cat.t()
    lora = torch.cat([t[:, g * r:(g + 1) * r] @ B.t() for g, B in enumerate(Bs)], 1)
    y = x @ W.t() + scale * lora
    return (y if res is None else res + y), t
