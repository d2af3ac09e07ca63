"""A float64 model of the attention entry points (include/set_amd.h: set_attention, set_attention_bwd, set_bmm, set_softmax_rows(_bwd),
set_make_positions, set_head_mean, set_mask_fill_chan, set_masked_channel_sum), written from the comments of the header and not from the
kernels, the case tables of the GPU branch sweep tests/test_gpu_attention_branches.py, and the CPU half of its argument: the model against
torch in float64, the inventory (every branch of csrc/attention_fused.hip and csrc/attention.hip has a case whose C condition is asserted
from the case's numbers), the conditions `exact` mode rests on, and the derived bar of `bounded` mode against the tolerances of
test_fused_attention_forward_and_gradients.

Semantics of the model.  A padded key (kpm != 0) has the constant score `fill`: dq and dk get nothing from it, dv does (p dO).  Keys beyond
Tk do not exist.  fill = -inf and every key padded: m = -inf, l = 0, o = p = NaN (torch's softmax of an all -inf row); fill = -1e8 and
every key padded: uniform over all Tk keys.  bf16 mode: the operands are the bf16-rounded alpha q, k, v, dO (delta = sum_c dO o stays fp32).

exact mode (fused kernels).  Query and key frames carry class codes: +-1 over all d channels, rows of a Hadamard matrix of order d (32, 64:
Sylvester; 96 = H12 (x) H8; a key adds a second row from the half of the matrix no query uses, so that keys of one class differ and
dq is not identically zero), and alpha is a power of two with g = alpha d >= 128.  A score is g for equal classes and 0 otherwise, so
s - m is one of 0, -g, fill - m, and exp(-g) < 2^-149: every exp is exactly 0 or 1 in fp32, every rescale factor of an online softmax is
0 or 1 in whatever order the tiles arrive, l is the integer count of the keys at the maximum, m is g or 0 (or fill).  v and dO are small
integers, a query matches n in {1, 2, 4, 8} keys before masking.  Then, asserted per case by exact_conditions():
  * m, l bit for bit; p = fl32(1 / l) on the keys at the maximum and 0 elsewhere -- the build divides with v_div_scale / v_rcp / v_div_fixup
    (IEEE, correctly rounded; checked in the gfx950 assembly of attention_fused.hip: no fast-math flag, -ffp-contract=off), and
    __expf(0) = 1, __expf(x <= -128) = 0 (v_mul by log2 e, v_exp_f32: 2^0 and an underflow);
  * o bit for bit where l is a power of two; where it is not (queries that match no key: l = the count of unpadded keys, which is what
    catches an unmasked partial tile; classes thinned by a mask to 3, 5, ... keys) o = fl(acc) fl(1 / l) is held to 3 u |o|;
  * dO is zero on every query whose l is not a power of two, so P (1 / n) and dS = P (dP - delta) are dyadic with few bits and delta, dq,
    dk, dv are exact sums: every sum of absolute terms stays below 2^24 granules;
  * bf16: alpha q, k, v, dO and the kernel-internal P and dS (rounded to bf16 for the second GEMMs) are representable in 8 significand
    bits.  Where a case's dS is not, its bf16 backward is compared in bounded mode only (column `bf16 bwd` of test_exact_inventory).

bounded mode.  Gaussian q, k, v, dO with alpha = c / sqrt(d), c in SCALES: N(0, 1) scores and two wider ones.  Ordered cases add a score
offset of STEP per 32-key tile through channel 0 of every head (q = 1, k = offset / alpha, the same for every query): rising, the running
maximum grows by STEP in every live tile, so every rescale factor is near exp(-STEP); falling, the maximum sits in the first live tile
and a tail of exp(s - m) down to underflow follows.  These reach scores tens of units apart (asserted: more than 20) while the keys that
carry the probability keep scores of the size of the unordered cases.  Every element is held to a bar derived from the case's own data
(attn_bars), nothing clamped.  The rounding model: one fp32 rounding of a value v is an error uniform in [-u |v|, u |v|], u = 2^-24,
standard deviation u |v| / sqrt(3); errors of different roundings are independent, a sum of them is held to six standard deviations,
KSIG u sqrt(sum v^2) with KSIG = 6 / sqrt(3) = 3.5 (about 1e7 elements are compared in a run; six sigma leaves 2e-9 each).  Terms that
need not be zero-mean (exp, the bf16 rounding of P and dS) are added linearly at their worst case.  Per (b, head), query i, key j:
  chain(Q, S) = KSIG u sqrt(d (Q / 6 + S^2 / 3) + S^2 + Q): a dot product of d terms with sum S and sum of squared products Q, added in an
                order the model does not know: the partial sum after t of d terms has mean square (t / d)(1 - t / d) Q + (t / d)^2 S^2, which
                sums to d (Q / 6 + S^2 / 3); one more rounding of the result and of each operand (alpha q).  Two MFMA chains of d / 2 and
                their join give less, bf16 products are exact in fp32 and summed in fp32: the same bound serves all.
  score      ds_ij  = chain(sum_c (alpha q_ic k_jc)^2, s_ij); a padded key's score is the constant fill: 0.
  exp        ex_ij  = 2^-23 (1 + 1.5 |x|) + 2 u, x = s - m: v_exp_f32 is accurate to 1 ulp (AMD's public CDNA ISA guide, table of
                      transcendental precision; the guides beside this repository state none), __expf(x) = exp2(x log2 e) rounds the
                      product and the constant (2 u |x| relative) and x itself is a rounded difference (u |x|).  Keys with p = 0 carry none.
  keys       g_k    = KSIG u sqrt(Tk + ceil(Tk / 32)): one rounding per key and one rescale per tile on a partial sum that never exceeds
                      the whole (terms >= 0 for l; against sum p |v| for o).  g_q likewise over Tq.
  l          epsl_i = sqrt(sum_j (p_ij ds_ij)^2) + sum_j p_ij ex_ij + g_k       relative; the shift of the stored m cancels between e and l
  stored m, l       |m^ - m| <= max ds over the keys within 0.5 of the maximum; the stored l also moves with the stored m
  p          p_ij (ds_ij + ex_ij + epsl_i + 3 u): the probabilities kernel contracts the scores again, in another order, and divides by the
             forward's l, so the two score errors do not cancel (Tq = Tk = 1: p^ = exp(s' - s^) need not be 1)
  o          o^_c - o_c = sum_j p_j eta_j (v_jc - o_c), eta the relative error of e_j: what is common to a row's keys cancels.
             do_ic = sqrt(sum_j (p_ij ds_ij (v_jc - o_ic))^2) + sum_j p_ij ex_ij (|v_jc| + |o_ic|) + g_k (sum_j p_ij |v_jc| + |o_ic|) + 2 u |o_ic|
             bf16: + 2^-8 sum_{j: x_ij != 0} p_ij |v_jc| (the unnormalised P is rounded to 8 significand bits, truncation allowed for;
             exp(0) = 1 at the row maximum is representable; l sums the fp32 values)
  backward   D_ij = dP_ij - delta_i;  d(dP)_ij = chain(sum_c (dO_ic v_jc)^2, dP_ij)
             d(delta)_i = sqrt(sum_j (p_ij ds_ij D_ij)^2) + sum_j p_ij ex_ij |D_ij|   (sum_c dO_ic (o^_ic - o_ic) = sum_j p_j eta_j D_ij)
                          + sqrt(sum_c (dO_ic acc_ic)^2) + chain over c of dO o  [+ bf16: 2^-8 sum_{x != 0} p |dP|]
             dS^ - dS: independent from key to key   p_ij sqrt(ds_ij^2 D_ij^2 + d(dP)_ij^2)       (P recomputed from new scores)
                       common to a query's keys       (epsl_i + 4 u) |dS_ij| + p_ij d(delta)_i     (the stored l; delta)
                       linear                         p_ij ex_ij |D_ij| + (2 u + [bf16: 2^-8]) |dS_ij|;   0 on a padded key
             dq: the independent part in quadrature over j against k_jc^2; d(delta)_i |sum_j p_ij k_jc|; (epsl_i + 4 u) |dq|; the linear
                 part and g_k against sum_j |dS_ij| |k_jc|; all times alpha
             dk: independent and per-query parts in quadrature over i against (alpha q_ic)^2; linear part and g_q against sum_i |dS| |alpha q|
             dv: sqrt(sum_i (p_ij (ds_ij + epsl_i + 4 u) dO_ic)^2) + sum_i p_ij (ex_ij + [bf16: 2^-8] + g_q) |dO_ic| + 2 u |dv|
The tolerances of test_fused_attention_forward_and_gradients stay an upper cap, cap = 2e-5 max(1, max |want|) for o, 1e-5 for p, 5e-5 max(1,
max |want|) for dq / dk / dv (bf16: 2e-2, 2e-2, 3e-2): test_bounded_bar_is_never_looser_than_the_existing_tolerances asserts that the largest
derived value of every output of every case, unclamped, is at or below its cap, and prints the ratio.  The caps decide two things about
the cases.  (1) p in fp32: on a row that one key dominates, p moves by that key's score error, about 20 u |s| at d = 96 at six sigma, twice
over (the forward's l, the probabilities kernel's own scores), so 1e-5 admits |s| up to about 4: N(0, 1) scores and no wider.  p is asked
for in bounded mode on the N(0, 1) cases only (make_fused()["want_p"]); at the wider scales the call passes p = NULL and the p buffer must
keep its sentinel.  Exact mode asks for p on every case marked want_p.  (2) SCALES stops at 2.4, where the bars of o, dq, dk, dv reach
about 0.7 of their caps; the ordered cases carry the wide spreads.  A key class that every query of a long Tq puts all its weight on
(all but one key padded) collects Tq independent d(dP) errors in one dk row: that mask runs at Tq = 33."""
import functools
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
NEG_INF = float("-inf")
SCALES = (1.0, 1.7, 2.4)
STEP = 16.0  # ordered cases: the score offset between one 32-key tile and the next
KSIG = 3.5   # six standard deviations of a rounding error uniform in [-u |v|, u |v|]: 6 / sqrt(3)
MASK_ON, MASK_OFF = (1.0, 0.5, -1.0), (0.0, -0.0)  # "!= 0 = padded": every value the header's sentence covers
CAPS = {"f32": dict(o=2e-5, p=1e-5, dq=5e-5, dk=5e-5, dv=5e-5), "bf16": dict(o=2e-2, p=2e-2, dq=3e-2, dk=3e-2, dv=3e-2)}


# ------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------
def _split(t, heads):
    B, H, T = t.shape
    return t.reshape(B, heads, H // heads, T).transpose(2, 3)  # [B, heads, T, d]


def _join(t):
    B, h, T, d = t.shape
    return t.transpose(2, 3).reshape(B, h * d, T)


def _bf16(t):
    return t.float().bfloat16().double()


def attn_model(q, k, v, kpm, fill, alpha, heads, do=None, bf16=False, flush=False):
    """q [B, H, Tq], k, v [B, H, Tk] fp32 (channel-major, head h = channels [h d, (h + 1) d)), kpm [B, Tk] or None.  flush: exp below the
    smallest fp32 subnormal is 0 (what fp32 arithmetic gives; exact mode).  Returns float64 tensors in the layouts of the entry points."""
    r = _bf16 if bf16 else (lambda t: t.double())
    qs = _split(r(q.float() * alpha) if bf16 else q.double() * alpha, heads)
    kh, vh = _split(r(k), heads), _split(r(v), heads)
    s = qs @ kh.transpose(2, 3)
    pad = None
    if kpm is not None:
        pad = (kpm != 0)[:, None, None, :].expand_as(s)
        s = torch.where(pad, torch.tensor(float(fill), dtype=torch.float64), s)
    m = s.max(-1).values
    x = s - m[..., None]
    e = torch.exp(x)
    if flush:
        e = torch.where(x < -104.0, torch.zeros_like(e), e)
    l = torch.where(m == NEG_INF, torch.zeros_like(m), e.sum(-1))
    p = e / l[..., None]
    o = (e @ vh) / l[..., None]  # (normalised last: an integer sum that cancels to 0 stays 0 whatever l is)
    out = dict(o=_join(o), m=m, l=l, lse=torch.stack([m, l], 2), p=p, s=s, x=x, pad=pad, qs=qs, kh=kh, vh=vh)
    if do is not None:
        doh = _split(r(do), heads)
        dP = doh @ vh.transpose(2, 3)
        delta = (_split(do.double(), heads) * o).sum(-1)
        dS = p * (dP - delta[..., None])
        if pad is not None:
            dS = torch.where(pad, torch.zeros_like(dS), dS)
        out.update(delta=delta, dS=dS, dP=dP, doh=doh, dq=_join(alpha * (dS @ kh)), dk=_join(dS.transpose(2, 3) @ qs), dv=_join(p.transpose(2, 3) @ doh))
    return out


def _torch_attention(q, k, v, kpm, fill, alpha, heads, do):
    with torch.enable_grad():
        qh, kh, vh = (_split(t.double(), heads).detach().requires_grad_(True) for t in (q, k, v))
        sc = alpha * (qh @ kh.transpose(2, 3))
        if kpm is not None:
            sc = sc.masked_fill((kpm != 0)[:, None, None, :], fill)
        pr = torch.softmax(sc, -1)
        o = _join(pr @ vh)
        o.backward(do.double())
    return o.detach(), pr.detach(), torch.logsumexp(sc, -1).detach(), _join(qh.grad), _join(kh.grad), _join(vh.grad)


MODEL_VS_TORCH = [  # B, heads, d, Tq, Tk, fill, padded keys per utterance
    (2, 2, 8, 5, 7, NEG_INF, None), (2, 1, 4, 9, 6, NEG_INF, [2, 0]), (2, 2, 8, 3, 40, -1e8, [7, 39]), (3, 2, 4, 6, 5, -1e8, [1, 5, 0]),
    (2, 1, 16, 1, 1, NEG_INF, None), (2, 2, 4, 7, 9, NEG_INF, [9, 3]),
]


@pytest.mark.parametrize("case", MODEL_VS_TORCH)
def test_model_equals_torch_in_float64(case):
    B, heads, d, Tq, Tk, fill, npad = case
    g = torch.Generator().manual_seed(Tq * 11 + Tk)
    q, k, v, do = (torch.randn(B, heads * d, T, generator=g) for T in (Tq, Tk, Tk, Tq))
    kpm = None
    if npad is not None:
        kpm = torch.zeros(B, Tk)
        for b, n in enumerate(npad):  # scattered, not a tail
            kpm[b, torch.randperm(Tk, generator=g)[:n]] = torch.tensor(MASK_ON)[torch.arange(n) % 3]
    alpha = 1.7 * d ** -0.5
    mo = attn_model(q, k, v, kpm, fill, alpha, heads, do)
    o, pr, lse, dq, dk, dv = _torch_attention(q, k, v, kpm, fill, alpha, heads, do)
    nan_b = torch.isnan(o).flatten(1).any(1)
    assert nan_b.tolist() == [fill == NEG_INF and npad is not None and n == Tk for n in (npad or [0] * B)]
    ok = ~nan_b
    for name, want in (("o", o), ("p", pr), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert float((mo[name][ok] - want[ok]).abs().max()) < 1e-12, name
    assert float((mo["m"][ok] + torch.log(mo["l"][ok]) - lse[ok]).abs().max()) < 1e-12
    # the fully padded utterance under -inf, as torch has it: o, p, dv NaN, dq and dk exactly 0 (masked_fill passes no gradient)
    for b in nan_b.nonzero().flatten().tolist():
        assert bool(torch.isnan(mo["o"][b]).all()) and bool(torch.isnan(mo["p"][b]).all()) and bool(torch.isnan(mo["dv"][b]).all())
        assert bool(torch.isnan(dv[b]).all()) and bool((dq[b] == 0).all()) and bool((dk[b] == 0).all())
        assert bool((mo["dq"][b] == 0).all()) and bool((mo["dk"][b] == 0).all())
        assert bool((mo["m"][b] == NEG_INF).all()) and bool((mo["l"][b] == 0).all()) and bool(torch.isnan(mo["delta"][b]).all())
    if fill == -1e8 and npad is not None:
        for b, n in enumerate(npad):
            if n == Tk:  # uniform over all Tk keys
                assert bool((mo["p"][b] == 1.0 / Tk).all()) and bool((mo["l"][b] == Tk).all()) and bool((mo["m"][b] == -1e8).all())


# ------------------------------------------------------------------------------------------------------------------------
# fused attention: the case table
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def hadamard(n):
    """+-1 matrix of order n with orthogonal rows: Sylvester for powers of two, H12 (x) H8 for 96."""
    if n == 1:
        return np.ones((1, 1))
    if n == 12:  # Paley I, q = 11
        qr = {(i * i) % 11 for i in range(1, 11)}
        Q = np.array([[0 if i == j else (1 if (j - i) % 11 in qr else -1) for j in range(11)] for i in range(11)], dtype=np.float64)
        S = np.zeros((12, 12))
        S[0, 1:], S[1:, 0], S[1:, 1:] = 1, -1, Q
        h = S + np.eye(12)
    elif n % 12 == 0 and n & (n - 1):
        h = np.kron(hadamard(12), hadamard(n // 12))
    else:
        h = np.kron(np.array([[1.0, 1.0], [1.0, -1.0]]), hadamard(n // 2))
    assert h.shape == (n, n) and np.array_equal(h @ h.T, n * np.eye(n)) and bool((np.abs(h) == 1).all())
    return h


def _case(name, B, heads, Tq, Tk, mask, fill, layout, branch, cond, n=2, place="block", want_p=True, scale=0, order=None, dims=(32, 64, 96),
          bf16_bwd_bounded_only=()):
    return dict(bf16_bwd_bounded_only=bf16_bwd_bounded_only, name=name, B=B, heads=heads, Tq=Tq, Tk=Tk, mask=mask, fill=fill, layout=layout, branch=branch, cond=cond, n=n, place=place,
                want_p=want_p, scale=scale, order=order, dims=dims)


# mask: None | ("tail", [n per b]) | ("lead", [n per b]) | ("block", lo, hi) | ("scatter", every) | ("allbut", kept key) ; an entry of Tk
# in tail / lead = a fully padded utterance.  layout: packed (q, k, v slices of one [B, 3H, T]), separate (q dense, k, v slices of one
# [B, 2H, Tk]), strided (everything a frame slice of longer rows in its own allocation, every stride different).
# scale: index into SCALES for bounded mode.  cond: the C condition, evaluated by test_fused_inventory with the case's numbers.
FUSED = [
    _case("one_by_one", 2, 2, 1, 1, None, NEG_INF, "separate", "ntiles == 1, qc clamp on every lane but one", "Tq == 1 and Tk == 1 and (Tk + 31) // 32 == 1", n=1),
    _case("q33_k19_tail_full_1e8", 3, 2, 33, 19, ("tail", [5, 0, 19]), -1e8, "separate", "partial single tile: code-2 keys; a fully padded utterance is uniform",
          "Tk < 32 and 19 in mask[1] and fill == -1e8 and Tq == 33", n=2, scale=1),
    _case("q127_k32_scatter", 2, 2, 127, 32, ("scatter", 3), NEG_INF, "separate", "one whole tile, no code 2; codes scattered over both lane halves",
          "Tk == 32 and Tq == 127 and Tq % 128 == 127 and mask[0] == 'scatter'", n=4, place="stride"),
    _case("q33_k33_allbut", 2, 2, 33, 33, ("allbut", 32), NEG_INF, "strided", "second tile holds one key, and it is the only live one: dead through tile 0",
          "Tk == 33 and mask[1] >= 32", n=1, scale=0),
    _case("q129_k64_full_inf", 2, 2, 129, 64, ("tail", [64, 9]), NEG_INF, "separate", "a fully padded utterance under -inf beside a normal one: NaN, (m, l) = (-inf, 0)",
          "Tk == 64 and Tq == 129 and Tq > 128 and mask[1][0] == Tk and fill == NEG_INF", n=2, scale=1),
    _case("q261_k100_lead_inf", 2, 2, 261, 100, ("lead", [33, 67]), NEG_INF, "separate", "dead = (mn == -inf): the first whole tile(s) padded with -inf, live keys follow",
          "min(mask[1]) >= 33 and fill == NEG_INF and Tq > 256 and Tq % 128 != 0 and Tk == 100", n=4),
    _case("q33_k100_lead_1e8", 2, 2, 33, 100, ("lead", [33, 67]), -1e8, "strided", "the same leading mask with the finite fill: m starts at -1e8, corr = exp(-1e8 - mn) = 0",
          "min(mask[1]) >= 33 and fill == -1e8", n=4, scale=2, order="falling"),
    _case("self_t100_block", 2, 2, 100, 100, ("block", 30, 70), NEG_INF, "packed", "self-attention packing; an interior block of padded keys across two tile edges",
          "layout == 'packed' and mask[1] < 32 < 64 < mask[2] < Tk", n=2, want_p=False, scale=1, order="rising"),
    _case("q128_k64_full_1e8_pow2", 2, 2, 128, 64, ("tail", [64, 10]), -1e8, "strided", "fully padded under -1e8 with Tk a power of two: dv of padded keys exact, dk exactly 0",
          "Tk == 64 and Tq == 128 and mask[1][0] == Tk and fill == -1e8", n=8, scale=0),
    _case("self_t65_none", 2, 2, 65, 65, None, NEG_INF, "packed", "no mask (kpm == NULL); third tile holds one key", "mask is None and Tk == 65 and order == 'falling'", n=8, place="stride", scale=2, order="falling",
          bf16_bwd_bounded_only=(96,)),  # dS = (dP - delta) / 8 with |dP - delta| up to 45: more than 8 significand bits at d = 96
    _case("q40_k96_every_slot", 2, 2, 40, 96, ("scatter", 5), -1e8, "strided", "n = 1 classes on all 32 register slots of af_row (16 per lane half) in three tiles, among padded keys",
          "Tk % 32 == 0 and n == 1 and place == 'slot'", n=1, place="slot", want_p=False, scale=1),
    _case("self_t800", 2, 2, 800, 800, None, NEG_INF, "packed", "the CampNet self-attention shape: 25 key tiles, 7 query blocks", "Tq == 800 and Tk == 800", n=8, place="stride",
          want_p=False, dims=(96,), bf16_bwd_bounded_only=(96,)),
]
FUSED_RUNS = [(c, d) for c in FUSED for d in c["dims"]]
FUSED_IDS = ["%s-d%d" % (c["name"], d) for c, d in FUSED_RUNS]


def make_mask(c):
    B, Tk, mk = c["B"], c["Tk"], c["mask"]
    if mk is None:
        return None
    on = torch.zeros(B, Tk, dtype=torch.bool)
    if mk[0] == "tail":
        for b, n in enumerate(mk[1]):
            on[b, Tk - n:] = n > 0
    elif mk[0] == "lead":
        for b, n in enumerate(mk[1]):
            on[b, :n] = True
    elif mk[0] == "block":
        on[:, mk[1]:mk[2]] = True
        on[B - 1, mk[1] + 3] = False  # a live key inside the block
    elif mk[0] == "scatter":
        for b in range(B):
            on[b, (torch.arange(Tk) * 7 + b) % mk[1] == 0] = True
    elif mk[0] == "allbut":
        on[:] = True
        for b in range(B):
            on[b, mk[1] - b] = False
    idx = torch.arange(B * Tk).view(B, Tk)
    return torch.where(on, torch.tensor(MASK_ON)[idx % 3], torch.tensor(MASK_OFF)[idx % 2])


def exact_alpha(d):
    return {32: 4.0, 64: 2.0, 96: 2.0}[d]


def _pow2(t):
    return (t > 0) & (torch.frexp(t)[0] == 0.5)


def _rep32(t):
    f = torch.isfinite(t)
    return bool((t[f].float().double() == t[f]).all())


def _rep_bf16(t):
    return bool((_bf16(t) == t).all())


@functools.lru_cache(None)
def make_fused(name, d, mode):
    """Operands (fp32, channel-major), the model's outputs for fp32 and bf16 operands, and the per-element bars.  One build per case."""
    c = next(x for x in FUSED if x["name"] == name)
    B, heads, Tq, Tk, n = c["B"], c["heads"], c["Tq"], c["Tk"], c["n"]
    H = heads * d
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in name) * 13 + d + (mode == "exact"))
    kpm = make_mask(c)
    out = dict(c=c, d=d, kpm=kpm, mode=mode)
    if mode == "exact":
        alpha = exact_alpha(d)
        had = torch.from_numpy(hadamard(d)).float()
        ncls = min(d // 2, max(1, Tk // n))                        # class rows [0, d / 2); rows [d / 2, d - 2) are the keys' second component
        kcls = torch.full((B, heads, Tk), d - 2, dtype=torch.long)  # filler class: no query has it
        for b in range(B):
            for h in range(heads):
                for j in range(ncls):
                    for i in range(n):
                        t = (j * n + i + 3) % Tk if c["place"] == "block" else (j + i * ncls + 3 + (ncls * h if c["place"] == "slot" else 0)) % Tk
                        kcls[b, h, t] = (j + 7 * b + 3 * h) % ncls
        tq = torch.arange(Tq)
        qcls = torch.where(tq % 4 == 3, torch.tensor(d - 1), (tq * 5 + 1) % ncls).expand(B, heads, Tq)  # class d - 1: matches no key
        q = had[qcls].permute(0, 1, 3, 2).reshape(B, H, Tq).contiguous()
        # keys of one class would all be the same vector and dq = alpha sum_j dS_j k_j = 0 (sum_j dS_j = 0): every key adds a row of its own
        # from the half no query uses -- orthogonal to every query, so no score changes, and dq = alpha sum_j dS_j aux_j is not zero
        aux = d // 2 + (torch.arange(Tk) * 3 + 1) % (d // 2 - 2)
        k = (had[kcls] + had[aux]).permute(0, 1, 3, 2).reshape(B, H, Tk).contiguous()
        v = torch.randint(-3, 4, (B, H, Tk), generator=g).float()
        do = (torch.randint(-2, 3, (B, H, Tq), generator=g) * (torch.rand(B, H, Tq, generator=g) < 0.125)).float()
        fwd = attn_model(q, k, v, kpm, c["fill"], alpha, heads, flush=True)
        keep = _pow2(fwd["l"])  # [B, heads, Tq]: dO only where 1 / l is exact
        do = do * keep[:, :, None, :].expand(B, heads, d, Tq).reshape(B, H, Tq)
        m32 = attn_model(q, k, v, kpm, c["fill"], alpha, heads, do, flush=True)
        out.update(q=q, k=k, v=v, do=do, alpha=alpha, want={"f32": m32, "bf16": m32}, keep=keep, want_p=c["want_p"], ncls=ncls, qcls=qcls, kcls=kcls)
        out["bars"] = {dt: exact_bars(out, m32) for dt in ("f32", "bf16")}
    else:
        alpha = SCALES[c["scale"]] * d ** -0.5
        q, k, v, do = (torch.randn(B, H, T, generator=g) for T in (Tq, Tk, Tk, Tq))
        if c["order"]:  # channel 0 of every head carries a score offset of STEP per 32-key tile, the same for every query
            nt = (Tk + 31) // 32
            tile = (torch.arange(Tk) // 32).expand(B, Tk)
            first = torch.zeros(B, 1, dtype=torch.long) if kpm is None else ((kpm == 0).float().argmax(1, keepdim=True) // 32)  # first live tile
            off = -STEP * ((nt - 1 - tile) if c["order"] == "rising" else (tile - first)).float()  # 0 on the tile that holds the maximum
            q[:, ::d, :] = 1.0
            k[:, ::d, :] = (off / alpha)[:, None, :]
        out.update(q=q, k=k, v=v, do=do, alpha=alpha, want={}, bars={}, want_p=c["want_p"] and c["scale"] == 0)
        for dt in ("f32", "bf16"):
            mo = attn_model(q, k, v, kpm, c["fill"], alpha, heads, do, bf16=dt == "bf16")
            out["want"][dt] = mo
            out["bars"][dt] = attn_bars(out, mo, dt)
    return out


def exact_bars(o, mo):
    """Zero everywhere, except o on the queries whose l is not a power of two: 3 u |o| (fl(fl(acc) fl(1 / l)): two roundings, 2 u + u^2)."""
    B, heads, Tq = mo["l"].shape
    loose = (~o["keep"])[:, :, None, :].expand(B, heads, o["d"], Tq).reshape(B, -1, Tq)
    bar_o = torch.where(loose, 3 * U * mo["o"].abs(), torch.zeros_like(mo["o"]))
    z = lambda n: torch.zeros_like(mo[n])
    return dict(o=torch.nan_to_num(bar_o, nan=0.0), lse=z("lse"), p=z("p"), delta=z("delta"), dq=z("dq"), dk=z("dk"), dv=z("dv"))


def exact_conditions(o):
    """What `exact` mode rests on, from the case's own numbers.  Returns whether the bf16 backward is exact too."""
    c, d, mo = o["c"], o["d"], o["want"]["f32"]
    alpha, g = o["alpha"], o["alpha"] * o["d"]
    assert g >= 128 and math.log2(alpha) == int(math.log2(alpha))
    live = torch.isfinite(mo["m"])
    s = mo["s"]
    fin = s[torch.isfinite(s)]
    assert bool(((fin == g) | (fin == 0) | (fin == c["fill"])).all())  # the three scores there are
    x = mo["x"][live]
    assert bool(((x == 0) | (x <= -128)).all())                        # every exp is 1 or an underflow
    l = mo["l"]
    assert bool((l == l.round()).all()) and float(l.max()) < 2 ** 24 and bool((l[live] >= 1).all())
    assert bool(((mo["m"] == g) | (mo["m"] == 0) | (mo["m"] == c["fill"])).all())
    assert bool((o["do"].view(c["B"], c["heads"], d, c["Tq"]).abs().sum(2)[~o["keep"]] == 0).all())  # dO only where 1 / l is exact
    # integer budgets, in granules: scores (alpha), the o accumulation (1), delta and P (2^-6: l <= 64 where dO != 0), dS and the gradients (2^-12)
    G6, G12 = 2.0 ** 6, 2.0 ** 12
    assert g < 2 ** 24 and float(o["v"].abs().sum(2).max()) < 2 ** 24
    dS, p = torch.nan_to_num(mo["dS"]), torch.nan_to_num(mo["p"])
    assert bool((dS * G12 == (dS * G12).round()).all())
    assert float(dS.abs().sum(-1).max()) * alpha * G12 < 2 ** 24 and float(dS.abs().sum(-2).max()) * alpha * G12 < 2 ** 24
    pk = p * (mo["doh"].abs().sum(-1) > 0)[..., None]  # the P that meets a non-zero dO
    assert bool((pk * G6 == (pk * G6).round()).all()) and float(mo["doh"].abs().sum(-2).max()) * G6 < 2 ** 24
    dlt = torch.nan_to_num(mo["delta"])
    assert bool((dlt * G6 == (dlt * G6).round()).all()) and float((_split(o["do"].double(), c["heads"]).abs() * 3).sum(-1).max()) * G6 < 2 ** 24
    for name in ("lse", "delta", "dq", "dk", "dv"):
        assert _rep32(mo[name]), name
    assert _rep32(torch.where(o["bars"]["f32"]["o"] == 0, mo["o"], torch.zeros_like(mo["o"])))
    # p: fl32(1 / l) is the claim (correctly rounded division), whatever l
    assert all(_rep_bf16(t) for t in (o["q"] * alpha, o["k"], o["v"], o["do"])) and _rep_bf16(pk)
    return _rep_bf16(dS)


def attn_bars(o, mo, dt):
    """The derived per-element bars of bounded mode (module docstring).  Nothing is clamped: `cap` is what
    test_bounded_bar_is_never_looser_than_the_existing_tolerances holds the largest derived value of each output to."""
    c, d = o["c"], o["d"]
    heads, Tq, Tk, alpha = c["heads"], c["Tq"], c["Tk"], o["alpha"]
    b8 = 2.0 ** -8 if dt == "bf16" else 0.0
    nn = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
    T = lambda t: t.transpose(2, 3)
    qs, kh, vh, doh = mo["qs"], mo["kh"], mo["vh"], mo["doh"]        # alpha q, k, v, dO   [B, h, T, d]
    oh, p, dS = nn(_split(mo["o"], heads)), nn(mo["p"]), nn(mo["dS"])  # (a NaN utterance has no bar: NaN must meet NaN, 0 must meet 0)
    pad = mo["pad"]
    zpad = (lambda t: t) if pad is None else (lambda t: torch.where(pad, torch.zeros_like(t), t))
    chain = lambda Q, S: KSIG * U * torch.sqrt(d * (Q / 6 + S * S / 3) + S * S + Q)
    ds = zpad(chain((qs * qs) @ T(kh * kh), qs @ T(kh)))             # a padded key's score is the constant fill
    x = torch.where(p > 0, nn(mo["x"]), torch.zeros_like(p))         # a key with p = 0 carries no error
    ex = 2.0 ** -23 * (1 + 1.5 * x.abs()) + 2 * U
    gk, gq = KSIG * U * math.sqrt(Tk + math.ceil(Tk / 32)), KSIG * U * math.sqrt(Tq + math.ceil(Tq / 32))
    pb = p * b8 * (x != 0)                                            # bf16: exp(0) = 1 at the row maximum is representable, every other P is rounded
    pds2 = (p * ds) ** 2
    epsl = torch.sqrt(pds2.sum(-1)) + (p * ex).sum(-1) + gk          # [B, h, Tq]
    near = (p > 0) & (x > -0.5)                                      # the keys that can hold the stored maximum
    dm = torch.where(near, ds, torch.zeros_like(ds)).max(-1).values
    bar = dict(lse=torch.stack([dm + U * nn(mo["m"]).abs(), nn(mo["l"]) * (epsl + dm + U)], 2))
    bar["p"] = p * (ds + ex + epsl[..., None] + 3 * U)
    va, pe = vh.abs(), p * ex
    sq = lambda t: torch.sqrt(t.clamp(min=0.0))
    acc_o = gk * (p @ va + oh.abs()) + 2 * U * oh.abs()
    do_ = sq(pds2 @ (vh * vh) - 2 * oh * (pds2 @ vh) + oh * oh * pds2.sum(-1, keepdim=True)) + pe @ va + oh.abs() * pe.sum(-1, keepdim=True) + pb @ va + acc_o
    bar["o"] = _join(do_)
    D = nn(mo["dP"] - mo["delta"][..., None])
    ddP = chain((doh * doh) @ T(vh * vh), mo["dP"])
    do_raw = _split(o["do"].double(), heads)
    ddelta = (sq((pds2 * D * D).sum(-1)) + (pe * D.abs()).sum(-1) + (pb * mo["dP"].abs()).sum(-1) + sq(((do_raw * acc_o) ** 2).sum(-1))
              + KSIG * U * sq(d * ((do_raw * oh) ** 2).sum(-1) / 6 + (d / 3 + 1) * nn(mo["delta"]) ** 2))
    bar["delta"] = ddelta
    ind2 = zpad(p * p * (ds * ds * D * D + ddP * ddP))             # independent from key to key and from query to query
    com = epsl + 4 * U                                                # common to a query's keys: the stored l
    aS, qa, ka, doa = dS.abs(), qs.abs(), kh.abs(), doh.abs()
    pl = zpad(p)
    bar["dq"] = _join(alpha * (sq(ind2 @ (kh * kh)) + zpad(pe * D.abs()) @ ka + ddelta[..., None] * (pl @ kh).abs() + (2 * U + b8 + gk) * (aS @ ka))
                      + (com[..., None] + 2 * U) * _split(nn(mo["dq"]), heads).abs())
    row2 = (com[..., None] * aS + pl * ddelta[..., None]) ** 2
    bar["dk"] = _join(sq(T(ind2 + row2) @ (qs * qs)) + T(zpad(pe * D.abs())) @ qa + (2 * U + b8 + gq) * (T(aS) @ qa) + 2 * U * _split(nn(mo["dk"]), heads).abs())
    bar["dv"] = _join(sq(T((p * (ds + com[..., None])) ** 2) @ (doh * doh)) + T(pe) @ doa + (b8 + gq) * (T(p) @ doa) + 2 * U * _split(nn(mo["dv"]), heads).abs())
    bar = {n_: nn(t) for n_, t in bar.items()}
    bar["derived_max"], bar["cap"] = {}, {}
    for name, cap in CAPS[dt].items():
        w = mo[name][torch.isfinite(mo[name])]
        bar["cap"][name] = cap * max(1.0, float(w.abs().max()) if w.numel() else 1.0)
        bar["derived_max"][name] = float(bar[name].max())
    return bar


def test_hadamard_codes_are_orthogonal():
    for n in (32, 64, 96):
        h = hadamard(n)
        assert np.array_equal(h @ h.T, n * np.eye(n))
        assert exact_alpha(n) * n >= 128


def _af_row(r, half):  # the header comment of attention_fused.hip: register r of a lane in half `half` holds key (r & 3) + 8 (r >> 2) + 4 half
    return (r & 3) + 8 * (r >> 2) + 4 * half


@pytest.mark.parametrize("c,d", FUSED_RUNS, ids=FUSED_IDS)
def test_exact_inventory(c, d):
    """The conditions of exact mode on every case, and what each case puts where: matched keys on both lane halves and (Tk >= 32) on every
    register slot, queries that match no key, and their l = the count of unpadded keys."""
    o = make_fused(c["name"], d, "exact")
    bf16_bwd_exact = exact_conditions(o)
    mo = o["want"]["f32"]
    B, heads, Tq, Tk = c["B"], c["heads"], c["Tq"], c["Tk"]
    live_keys = torch.full((B,), float(Tk)) if o["kpm"] is None else (o["kpm"] == 0).sum(1).double()
    unmatched = (o["qcls"] == d - 1)
    if Tq > 1:
        assert bool(unmatched.any())
    for b in range(B):
        lb = mo["l"][b][unmatched[b]]
        if live_keys[b] > 0:
            assert bool((lb == live_keys[b]).all()) and bool((mo["m"][b][unmatched[b]] == 0).all())
        elif c["fill"] == -1e8:
            assert bool((mo["l"][b] == Tk).all()) and bool((mo["m"][b] == -1e8).all())
        else:
            assert bool((mo["l"][b] == 0).all()) and bool((mo["m"][b] == NEG_INF).all()) and bool(torch.isnan(mo["o"][b]).all())
    # keys that some query attends to with p > 0, by tile slot
    hit = (torch.nan_to_num(mo["p"]) > 0).any(2)  # [B, heads, Tk]
    slots = {(int(t) % 32) for t in hit.any(0).any(0).nonzero().flatten()}
    halves = {h for h in (0, 1) for r in range(16) if _af_row(r, h) in slots}
    assert halves == ({0, 1} if Tk >= 8 else {0})
    if Tk >= 32 and c["mask"] is None:
        assert slots == set(range(32))  # every register slot of af_row, in both lane halves
    if c["place"] == "slot":  # what the case's name promises, per lane half, and padded keys in every tile it uses
        for half in (0, 1):
            assert {_af_row(r, half) for r in range(16)} <= slots
        assert slots == set(range(32)) and all(bool((o["kpm"][:, t:t + 32] != 0).any()) for t in range(0, Tk, 32))
    nz = lambda t: int((torch.nan_to_num(t) != 0).sum())
    print("%s d%d: l in %s, non-zero o %d dq %d dk %d dv %d, NaN o %d; bf16 bwd %s" % (
        c["name"], d, sorted({int(v) for v in mo["l"].flatten().tolist()})[:8], nz(mo["o"]), nz(mo["dq"]), nz(mo["dk"]), nz(mo["dv"]),
        int(torch.isnan(mo["o"]).sum()), "exact" if bf16_bwd_exact else "bounded only (dS needs more than 8 bits)"))
    assert nz(mo["o"]) > 0 or bool(torch.isnan(mo["o"]).any())
    if c["n"] >= 2 and c["name"] != "q33_k33_allbut":
        assert nz(mo["dq"]) > 0 and nz(mo["dk"]) > 0 and nz(mo["dv"]) > 0
    assert bf16_bwd_exact == (d not in c["bf16_bwd_bounded_only"])


def bf16_bwd_exact(c, d):
    return d not in c["bf16_bwd_bounded_only"]


def test_fused_inventory():
    """Every branch the issue lists has a case at every head size, and each case meets the C condition it names."""
    for c in FUSED:
        env = dict(c, NEG_INF=NEG_INF)
        assert eval(c["cond"], {}, env), (c["name"], c["cond"])
    for d in (32, 64, 96):
        cs = [c for c in FUSED if d in c["dims"]]
        assert {1, 33, 127, 128, 129, 261} <= {c["Tq"] for c in cs} and {1, 19, 32, 33, 64, 100} <= {c["Tk"] for c in cs}
        kinds = {(None if c["mask"] is None else c["mask"][0], c["fill"]) for c in cs}
        assert {(None, NEG_INF), ("tail", -1e8), ("tail", NEG_INF), ("lead", NEG_INF), ("lead", -1e8), ("block", NEG_INF), ("scatter", NEG_INF),
                ("allbut", NEG_INF)} <= kinds
        full = {c["fill"] for c in cs if c["mask"] and c["mask"][0] in ("tail", "lead") and c["Tk"] in c["mask"][1] and min(c["mask"][1]) < c["Tk"]}
        assert full == {NEG_INF, -1e8}                                     # a fully padded utterance beside a normal one, under each fill
        assert {c["want_p"] for c in cs} == {True, False} and {c["layout"] for c in cs} == {"packed", "separate", "strided"}
        assert {c["scale"] for c in cs} == {0, 1, 2} and {c["order"] for c in cs} >= {"rising", "falling"}
        assert any(c["order"] and c["mask"] is None for c in cs) and any(c["order"] and c["mask"] for c in cs)
        assert len({c["name"] for c in cs if c["want_p"] and c["scale"] == 0}) >= 3  # p in bounded mode: the N(0, 1) cases
        assert {c["n"] for c in cs} == {1, 2, 4, 8}
        vals = set()
        for c in cs:
            m = make_mask(c)
            if m is not None:
                vals |= {(float(v), math.copysign(1.0, float(v))) for v in m.flatten().tolist()}
        assert vals == {(1.0, 1.0), (0.5, 1.0), (-1.0, -1.0), (0.0, 1.0), (0.0, -1.0)}  # -0.0 is a live key
    assert [c["name"] for c in FUSED if c["Tq"] == 800 and c["Tk"] == 800 and 96 in c["dims"]] == ["self_t800"]
    # the dead branch: a whole leading tile of -inf keys, live keys behind it
    for c in FUSED:
        if c["mask"] and c["mask"][0] == "lead" and c["fill"] == NEG_INF:
            m = make_mask(c)
            assert bool((m[:, :32] != 0).all()) and bool((m[:, 32:] == 0).any(1).all())


@pytest.mark.parametrize("c,d", FUSED_RUNS, ids=FUSED_IDS)
def test_bounded_bar_is_never_looser_than_the_existing_tolerances(c, d):
    o = make_fused(c["name"], d, "bounded")
    for dt in ("f32", "bf16"):
        bar = o["bars"][dt]
        for name in CAPS[dt]:
            assert bool((bar[name] >= 0).all()) and bool(torch.isfinite(bar[name]).all())
        print("%s d%d %s: derived max / cap  %s" % (c["name"], d, dt, "  ".join("%s %.2f" % (n, bar["derived_max"][n] / bar["cap"][n]) for n in CAPS[dt])))
        for name in CAPS[dt]:  # the derivation itself, unclamped, against the tolerance of test_fused_attention_forward_and_gradients
            if name == "p" and not o["want_p"]:
                continue  # not asked for in this run (module docstring: p at the wider scales)
            assert bar["derived_max"][name] <= bar["cap"][name], (c["name"], d, dt, name, bar["derived_max"][name], bar["cap"][name])
    mo = o["want"]["f32"]
    x = mo["x"] if mo["pad"] is None else torch.where(mo["pad"], torch.zeros_like(mo["x"]), mo["x"])
    spread = float(-x[torch.isfinite(x)].min()) if bool(torch.isfinite(x).any()) else 0.0
    print("%s d%d: scores spread over %.1f units" % (c["name"], d, spread))
    if c["order"]:  # on the scores the kernel sees (padded keys excluded), for every query: the maximum of each live tile rises / falls
        live = torch.ones_like(mo["s"], dtype=torch.bool) if mo["pad"] is None else ~mo["pad"]
        sm = torch.where(live, mo["s"], torch.full_like(mo["s"], NEG_INF))
        tiles = [sm[..., t:t + 32].max(-1).values for t in range(0, c["Tk"], 32)]
        steps = 0
        for a, b_ in zip(tiles, tiles[1:]):
            both = torch.isfinite(a) & torch.isfinite(b_)
            steps += int(both.sum())
            assert bool((b_ > a)[both].all()) if c["order"] == "rising" else bool((b_ < a)[both].all())
            if c["order"] == "rising":  # the rescale factor exp(m_old - m_new) is far from 1
                assert bool(((b_ - a)[both] > 3.0).all())
        assert steps >= c["B"] * c["heads"] * c["Tq"] and spread > 20.0  # "tens of units apart"


# ------------------------------------------------------------------------------------------------------------------------
# attention.hip: bmm
# ------------------------------------------------------------------------------------------------------------------------
def tile_map(s_mn, s_k):
    """load_tile's choice, from the comment of bmm_kernel: 'mn' (mn fastest across lanes) if the mn stride is 1 or the k stride is not."""
    return "mn" if (s_mn == 1 or s_k != 1) else "k"


# name, n_outer, n_inner, M, N, K, A storage, B storage, alpha (exact, bounded), accumulate, branch
# A storage: "mk" = [M][K] rows (a_ks == 1), "km" = [K][M] (a_ms == 1), "pad" = [M][2 K] every other element (both strides != 1)
# B storage: "kn" = [K][N] (b_ns == 1), "nk" = [N][K] (b_ks == 1), "pad" likewise
BMM = [
    ("mapk_mapmn", 1, 1, 64, 64, 32, "mk", "kn", 1.0, False, "A: k-fastest map, B: mn-fastest map; one full tile, one K chunk"),
    ("mapmn_mapk", 2, 3, 65, 65, 33, "km", "nk", -2.0, False, "A: mn map, B: k map; M, N = 65: a second tile row / column of one element; K = 33: a chunk of one"),
    ("mapk_mapk", 1, 2, 130, 1, 19, "mk", "nk", 0.5, True, "both k maps; K < 32; N = 1; accumulate with alpha != 1"),
    ("mapmn_mapmn", 3, 1, 1, 130, 40, "km", "kn", 0.5, True, "both mn maps; M = 1; K % 32 != 0 above 32; accumulate"),
    ("both_strided", 2, 2, 64, 65, 64, "pad", "pad", 1.0, True, "s_mn != 1 and s_k != 1 on both: mn map; K = 64; accumulate with alpha = 1"),
    ("k1", 1, 1, 33, 70, 1, "mk", "kn", 4.0, False, "K = 1"),
]


def make_bmm(case, mode):
    name, no, ni, M, N, K, sa, sb, alpha, acc, _ = case
    nb = no * ni
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in name) + (mode == "exact"))
    if mode == "exact":
        A, Bm, C0 = (torch.randint(-3, 4, s, generator=g).float() for s in ((nb, M, K), (nb, K, N), (nb, M, N)))
    else:
        A, Bm, C0 = (torch.randn(s, generator=g) for s in ((nb, M, K), (nb, K, N), (nb, M, N)))
        alpha = alpha * 0.7
    want = alpha * (A.double() @ Bm.double()) + (C0.double() if acc else 0.0)
    if mode == "exact":
        assert float((A.abs().double() @ Bm.abs().double()).max()) * abs(alpha) + float(C0.abs().max()) < 2 ** 24 and _rep32(want)
        bar = torch.zeros_like(want)
    else:  # K products in one MFMA chain, alpha, the add
        bar = (K + 2) * U * abs(alpha) * (A.abs().double() @ Bm.abs().double()) + 2 * U * want.abs() + (U * C0.abs().double() if acc else 0.0)
    return dict(A=A, B=Bm, C0=C0, want=want, bar=bar, alpha=alpha)


def bmm_strides(case):
    name, no, ni, M, N, K, sa, sb = case[:8]
    a = {"mk": (K, 1), "km": (1, M), "pad": (2 * K, 2)}[sa]     # (a_ms, a_ks)
    b = {"kn": (N, 1), "nk": (1, K), "pad": (2 * N, 2)}[sb]     # (b_ks, b_ns)
    return a, b


def test_bmm_inventory():
    maps = set()
    for case in BMM:
        (a_ms, a_ks), (b_ks, b_ns) = bmm_strides(case)
        maps.add((tile_map(a_ms, a_ks), tile_map(b_ns, b_ks)))
        for mode in ("exact", "bounded"):
            make_bmm(case, mode)
    assert maps == {("mn", "mn"), ("mn", "k"), ("k", "mn"), ("k", "k")}
    Ks, Ms, Ns = ({c[i] for c in BMM} for i in (5, 3, 4))
    assert any(k < 32 for k in Ks) and any(k > 32 and k % 32 for k in Ks) and {1, 33, 64} <= Ks and {64, 65} <= Ms and {64, 65} <= Ns
    assert any(c[9] and c[8] != 1.0 for c in BMM) and any(c[2] > 1 for c in BMM) and any(c[9] and c[8] == 1.0 for c in BMM)
    assert any(c[6] == "pad" for c in BMM)  # s_mn != 1 and s_k != 1: the first map by its second condition


# ------------------------------------------------------------------------------------------------------------------------
# attention.hip: the small kernels
# ------------------------------------------------------------------------------------------------------------------------
SOFTMAX = [  # rows, cols, rows_per_batch, mask?, fill        (one wave per row, 4 rows per block, lanes stride the columns by 64)
    (5, 1, 1, False, NEG_INF), (7, 19, 7, True, NEG_INF), (6, 63, 3, True, -1e8), (4, 64, 2, True, NEG_INF), (9, 65, 3, True, -1e8), (3, 129, 1, False, NEG_INF),
    (10, 70, 5, True, NEG_INF),
]


def make_softmax(case, mode):
    rows, cols, rpb, masked, fill = case
    g = torch.Generator().manual_seed(rows * 31 + cols + (mode == "exact"))
    nb = rows // rpb
    assert nb * rpb == rows
    kpm = None
    if masked:
        on = torch.rand(nb, cols, generator=g) < 0.3
        on[0] = True  # a fully padded batch entry: NaN under -inf, uniform under -1e8
        on[-1, 0] = False
        idx = torch.arange(nb * cols).view(nb, cols)
        kpm = torch.where(on, torch.tensor(MASK_ON)[idx % 3], torch.tensor(MASK_OFF)[idx % 2])
    if mode == "exact":  # logits 0 or -200 with 1, 2 or 4 at the top: p is 1 / n or 0
        x = torch.full((rows, cols), -200.0)
        for r in range(rows):
            x[r, torch.randperm(cols, generator=g)[:min(cols, (1, 2, 4)[r % 3])]] = 0.0
        dp = torch.randint(-4, 5, (rows, cols), generator=g).float()
    else:
        x, dp = torch.randn(rows, cols, generator=g) * 4, torch.randn(rows, cols, generator=g)
    s = x.double()
    if kpm is not None:
        s = torch.where((kpm != 0).repeat_interleave(rpb, 0), torch.tensor(float(fill), dtype=torch.float64), s)
    m = s.max(1, keepdim=True).values
    xm = s - m
    e = torch.exp(xm)
    if mode == "exact":
        e = torch.where(xm < -104.0, torch.zeros_like(e), e)
    p = e / e.sum(1, keepdim=True)
    nsum = math.ceil(cols / 64) + 6  # per-lane chain and the six exchanges of a wave sum
    xa = torch.nan_to_num(torch.where(e > 0, xm, torch.zeros_like(xm)), nan=0.0).abs()
    if mode == "exact":
        cnt = e.sum(1, keepdim=True)
        ok = ~torch.isnan(cnt)
        assert bool((cnt[ok] == cnt[ok].round()).all())
        want_p, bar_p = (e / cnt).float().double(), torch.zeros_like(p)  # fl32(1 / n): IEEE division
    else:  # expf (1 ulp) of a rounded difference: u |x| relative; the sum; the division
        want_p, bar_p = p, torch.nan_to_num(p) * U * (nsum + 4 + 2 * xa + (torch.nan_to_num(p) * 2 * xa).sum(1, keepdim=True))
    # the backward (it takes no mask): on the fp32 softmax of the unmasked logits -- 1 / n or 0 in exact mode
    eu = torch.exp(x.double() - x.double().max(1, keepdim=True).values)
    if mode == "exact":
        eu = torch.where(eu < 1e-40, torch.zeros_like(eu), eu)
    pf = (eu / eu.sum(1, keepdim=True)).float()
    dot = (pf.double() * dp.double()).sum(1, keepdim=True)
    ds = pf.double() * (dp.double() - dot)
    if mode == "exact":
        assert bool((_pow2(pf.double()) | (pf == 0)).all()) and _rep32(ds)
        bar_ds = torch.zeros_like(ds)
    else:
        bar_ds = U * ((nsum + 3) * pf.double() * (pf.double() * dp.double().abs()).sum(1, keepdim=True) + 3 * ds.abs() + pf.double() * dp.double().abs())
    return dict(x=x, kpm=kpm, p=want_p, bar_p=bar_p, pf=pf, dp=dp, ds=ds, bar_ds=bar_ds)


def make_tokens(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, 4, (B, T), generator=g)
    tok[0] = 7                     # every lane non-zero: the (1 << 63) - 1 mask when T >= 64, the full carry
    if B > 1:
        tok[1] = 0                 # an all-zero row
    if B > 2 and T > 64:
        tok[2, :64] = 0            # an empty first chunk: the carry is 0, not 64
    return tok


def positions_ref(nz):
    return torch.cumsum(nz.long(), 1) * nz.long()


POSITIONS_T = (1, 63, 64, 65, 150, 200)  # one partial chunk, lane 63, exactly one chunk, a carry into one lane, three chunks, four
HEAD_MEAN = [(2, 1, 255), (3, 2, 256), (2, 4, 257), (1, 8, 600)]  # B, heads (a power of two: the mean of integers is exact), n
MASK_FILL = [(2, 3, 43), (1, 1, 256), (1, 1, 257), (3, 5, 100), (2, 80, 7)]  # B, C, T: B C T of 258, 256, 257, 1500, 1120
CHANNEL_SUM = [(1, 2, 255), (2, 3, 128), (3, 1, 257), (2, 80, 300)]  # B, C, T: B T of 255, 256, 771, 600 against the block of 256


def test_small_kernel_inventory():
    assert {63, 64, 65} <= set(POSITIONS_T) and max(POSITIONS_T) > 3 * 64 and min(POSITIONS_T) < 64
    tok = make_tokens(3, 200, 1)
    assert bool((tok[0] != 0).all()) and bool((tok[1] == 0).all()) and bool((tok[2, :64] == 0).all()) and bool((tok[2, 64:] != 0).any())
    want = positions_ref(tok != 0)
    assert want[0].tolist() == list(range(1, 201)) and int(want[1].sum()) == 0
    cols = {c[1] for c in SOFTMAX}
    assert {64, 129} <= cols and any(c < 64 for c in cols) and any(c[0] % 4 for c in SOFTMAX)
    for case in SOFTMAX:
        for mode in ("exact", "bounded"):
            make_softmax(case, mode)
    assert all(h & (h - 1) == 0 for _, h, _ in HEAD_MEAN) and any(B * n > 256 and (B * n) % 256 for B, _, n in HEAD_MEAN)
    assert {256, 257, 258} <= {B * C * T for B, C, T in MASK_FILL}
    assert any(B * T < 256 for B, _, T in CHANNEL_SUM) and any(B * T == 256 for B, _, T in CHANNEL_SUM) and any(B * T > 512 for B, _, T in CHANNEL_SUM)
