"""GPU branch sweep of the attention kernels: the 24 fused kernels of csrc/attention_fused.hip (forward, probabilities, dQ pass, dK / dV
pass at head size 32 / 64 / 96 in fp32 / bf16) and the kernels of csrc/attention.hip (strided batched GEMM, row softmax forward and
backward, positions, head mean, masked fill, masked channel sum), each case ONE set_attention / set_attention_bwd / set_bmm / ... call
against the float64 model of tests/test_attention_reference.py (where the case tables live, each case naming the branch it reaches and
the C condition it meets, and where the CPU half of the argument runs).  Same shape as tests/test_gpu_conv_branches.py: every output
(o, lse, p, delta, dq, dk, dv, C, ...) is a view inside a larger buffer filled with a sentinel and the WHOLE buffer is compared; operands
are checked unchanged after the call.  SetAttnArgs / SetAttnBwdArgs are filled by hand, so that what ops.attention_fused cannot express
runs too: o_cs > Tq and an o_bs that is not H o_cs, q / k / v as frame slices of longer rows surrounded by 3e4 (which may change nothing),
k and v from different allocations with different strides, dq_cs / dk_cs / dv_cs different from the forward's.  Two modes per case:
  exact    class-coded queries and keys (test_attention_reference.py): every exp is 0 or 1, l is an integer count, and m, l, p, delta, dq,
           dk, dv must equal the model BIT FOR BIT (o too wherever 1 / l is exact, else within 3 u |o|) -- a key paired with the wrong
           value, a shifted mask code, a lost tile, an unmasked key of a partial tile shows as a wrong integer.
  bounded  Gaussian inputs at three score scales and two key orderings, every element within the derived bar attn_bars().

Pinned NaN semantics (fill = -inf, one utterance fully padded; the same as torch in float64, test_model_equals_torch_in_float64): that
utterance's o, p, delta and dv are NaN, its stored (m, l) is (-inf, 0), its dq and dk are exactly 0 (a padded key's score is the constant
fill); every other utterance of the batch is exact / within the bar, gradients included.

Not swept, on purpose: the 2 GiB slice guard of attn_check.  A refusal test must stay harmless if the refusal fails to trigger, and the
kernel would then run with that stride; it is left to a reading of the code."""
import ctypes as C
import math

import pytest
import torch

import test_attention_reference as R
from test_gpu_conv_branches import E_INVALID, E_UNSUPPORTED, SENTINEL, _ALIVE, _L, _keep_launch_operands, _p, _report, _s, dev  # noqa: F401

pytestmark = pytest.mark.gpu

BIG = 3.0e4   # what surrounds a strided operand: finite, so that one stray read shows in a sum instead of hiding in a NaN compare
G = 64        # guard elements in front of and behind every view
WORST = {}    # (output, dtype) -> worst observed |d| / bar of bounded mode, printed by the last test of the module


def _specs(c, d):
    """(buffer, batch stride, channel stride, offset) of q, k, v, o (dO has o's strides), dq, dk, dv."""
    H, Tq, Tk = c["heads"] * d, c["Tq"], c["Tk"]
    if c["layout"] == "packed":
        T = Tq
        s = {n: ("x", 3 * H * T, T, G + i * H * T) for i, n in enumerate("qkv")}
        s.update({"d" + n: ("dx", 3 * H * T, T, G + i * H * T) for i, n in enumerate("qkv")})
    elif c["layout"] == "separate":
        s = dict(q=("q", H * Tq, Tq, G), k=("kv", 2 * H * Tk, Tk, G), v=("kv", 2 * H * Tk, Tk, G + H * Tk))
        s.update(dq=("dq", H * Tq, Tq, G), dk=("dkv", 2 * H * Tk, Tk, G), dv=("dkv", 2 * H * Tk, Tk, G + H * Tk))
    else:
        s = dict(q=("q", H * (Tq + 5) + 11, Tq + 5, G + 7), k=("k", H * (Tk + 3) + 2, Tk + 3, G + 5), v=("v", H * (Tk + 9), Tk + 9, G + 1))
        s.update(dq=("dq", H * (Tq + 2) + 3, Tq + 2, G + 2), dk=("dk", H * (Tk + 1), Tk + 1, G), dv=("dv", H * (Tk + 4) + 9, Tk + 4, G + 6))
    s["o"] = ("o", H * (Tq + 6) + 13, Tq + 6, G + 3) if c["layout"] == "strided" else ("o", H * Tq, Tq, G)
    return s


class _Bufs:
    """Flat CPU buffers by name, each large enough for every view placed in it plus a guard."""

    def __init__(self, c, d):
        self.B, self.H = c["B"], c["heads"] * d
        self.T = dict(q=c["Tq"], k=c["Tk"], v=c["Tk"], o=c["Tq"], dq=c["Tq"], dk=c["Tk"], dv=c["Tk"])
        self.specs = _specs(c, d)

    def size(self, buf):
        return max(off + (self.B - 1) * bs + (self.H - 1) * cs + self.T[n] + G for n, (b, bs, cs, off) in self.specs.items() if b == buf)

    def view(self, flat, n):
        _, bs, cs, off = self.specs[n]
        assert cs >= self.T[n] and bs >= (self.H - 1) * cs + self.T[n] and off + (self.B - 1) * bs + (self.H - 1) * cs + self.T[n] <= flat.numel() - G
        return flat.as_strided((self.B, self.H, self.T[n]), (bs, cs, 1), off)

    def make(self, names, fill, dtype=torch.float32):
        return {b: torch.full((self.size(b),), fill, dtype=dtype) for b in sorted({self.specs[n][0] for n in names})}


def _flat(n, fill=SENTINEL, dtype=torch.float32):
    return torch.full((G + n + G,), fill, dtype=dtype)


def _cmp(name, tag, got, want, bar, key=None):
    """Whole-buffer comparison; a NaN must meet a NaN and an infinity the same infinity."""
    got, want, bar = got.double().flatten(), want.flatten(), bar.flatten()
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    z = torch.zeros_like(want)
    g2, w2 = torch.where(same, z, got), torch.where(same, z, want)
    bad = _report(name, tag, g2, w2, bar)
    assert bad.numel() == 0, (name, tag, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), bar[bad[:8]].tolist())
    if key is not None and bool((bar > 0).any()):
        WORST[key] = max(WORST.get(key, 0.0), float(((g2 - w2).abs() / (bar + 1e-300))[bar > 0].max()))


def _attn_args(c, d, o, bufs, dbuf, dt, want_p):
    from set_amd import _lib
    a = _lib.SetAttnArgs()
    sp = bufs.specs
    for n in "qkv":
        setattr(a, n, _p(dbuf[sp[n][0]]) + 4 * sp[n][3])
        setattr(a, n + "_bs", sp[n][1])
        setattr(a, n + "_cs", sp[n][2])
    a.o, a.o_bs, a.o_cs = _p(dbuf["o"]) + 4 * sp["o"][3], sp["o"][1], sp["o"][2]
    a.lse = _p(dbuf["lse"]) + 4 * G
    a.p = _p(dbuf["p"]) + 4 * G if want_p else None
    a.kpm = _p(dbuf["kpm"]) if o["kpm"] is not None else None
    a.B, a.heads, a.head_dim, a.Tq, a.Tk = c["B"], c["heads"], d, c["Tq"], c["Tk"]
    a.scale, a.fill, a.bf16 = o["alpha"], c["fill"], int(dt == "bf16")
    return a


def _embed_want(flat_like, view, value, bar):
    want = torch.full(flat_like.shape, SENTINEL, dtype=torch.float64)
    b = torch.zeros(flat_like.shape, dtype=torch.float64)
    view(want).copy_(value)
    view(b).copy_(bar)
    return want, b


def _run_fused(dev, c, d, mode, dt):
    """One set_attention call and one set_attention_bwd call on the case; every buffer compared whole."""
    from set_amd import _lib
    o = R.make_fused(c["name"], d, mode)
    mo, bars = o["want"][dt], o["bars"][dt]
    B, heads, Tq, Tk = c["B"], c["heads"], c["Tq"], c["Tk"]
    bufs = _Bufs(c, d)
    cpu = bufs.make("qkv", BIG)
    for n in "qkv":
        bufs.view(cpu[bufs.specs[n][0]], n).copy_(o[n])
    cpu["do"] = torch.full((bufs.size("o"),), BIG)
    bufs.view(cpu["do"], "o").copy_(o["do"])
    if o["kpm"] is not None:
        cpu["kpm"] = o["kpm"].contiguous()
    cpu["o"] = torch.full((bufs.size("o"),), SENTINEL)
    cpu["lse"], cpu["p"], cpu["delta"] = _flat(B * heads * 2 * Tq), _flat(B * heads * Tq * Tk if o["want_p"] else 1), _flat(B * heads * Tq)
    cpu.update(bufs.make(("dq", "dk", "dv"), SENTINEL))
    dbuf = {n: t.to(dev) for n, t in cpu.items()}
    key = lambda n: (n, dt) if mode == "bounded" else None
    tag = "%s %s" % (dt, mode)

    a = _attn_args(c, d, o, bufs, dbuf, dt, o["want_p"])
    _lib.check(_L().set_attention(C.byref(a), _s()), "set_attention")
    torch.cuda.synchronize()
    for n in ("x", "q", "k", "v", "kv", "kpm", "do"):  # operands are read-only
        if n in cpu:
            assert torch.equal(dbuf[n].cpu(), cpu[n]) or n == "kpm" and torch.equal(dbuf[n].cpu().view(torch.int32), cpu[n].view(torch.int32)), n
    got_o = dbuf["o"].cpu()
    _cmp(c["name"] + ".o", tag, got_o, *_embed_want(got_o, lambda t: bufs.view(t, "o"), mo["o"], bars["o"]), key=key("o"))
    got_lse = dbuf["lse"].cpu()
    _cmp(c["name"] + ".lse", tag, got_lse, *_embed_want(got_lse, lambda t: t[G:-G].view(B, heads, 2, Tq), mo["lse"], bars["lse"]))
    got_p = dbuf["p"].cpu()
    if o["want_p"]:
        want_p = mo["p"].float().double() if mode == "exact" else mo["p"]  # exact: fl32(1 / l), the correctly rounded quotient
        pv = lambda t: t[G:-G].view(B, heads, Tq, Tk)
        _cmp(c["name"] + ".p", tag, got_p, *_embed_want(got_p, pv, want_p, bars["p"]), key=key("p"))
        gp = pv(got_p).double()
        rows, live = gp.sum(-1), torch.isfinite(mo["m"])
        slack = (bars["p"].sum(-1) + R.U * Tk)[live] if mode == "bounded" else R.U * Tk
        assert bool(((rows[live] - 1).abs() <= slack).all()), float((rows[live] - 1).abs().max())  # a distribution, within the bar's own sum
        if o["kpm"] is not None and c["fill"] == R.NEG_INF:
            padded = (o["kpm"] != 0)[:, None, None, :].expand_as(gp) & live[..., None]
            assert bool((gp[padded] == 0).all())  # a padded key's p is exactly 0 under the -inf fill
    else:
        assert bool((got_p == SENTINEL).all())
    dead_b = ~torch.isfinite(mo["m"]).flatten(1).all(1)
    for b in dead_b.nonzero().flatten().tolist():  # the pinned NaN semantics, said once more in plain words
        assert bool(torch.isnan(bufs.view(got_o, "o")[b]).all())
        st = got_lse[G:-G].view(B, heads, 2, Tq)[b]
        assert bool((st[:, 0] == R.NEG_INF).all()) and bool((st[:, 1] == 0).all())

    if mode == "exact" and dt == "bf16" and not R.bf16_bwd_exact(c, d):
        return o  # this case's dS needs more than 8 significand bits: its bf16 backward runs in bounded mode only
    g = _lib.SetAttnBwdArgs()
    g.fwd = _attn_args(c, d, o, bufs, dbuf, dt, False)
    g.d_o, g.delta = _p(dbuf["do"]) + 4 * bufs.specs["o"][3], _p(dbuf["delta"]) + 4 * G
    for n in ("dq", "dk", "dv"):
        setattr(g, n, _p(dbuf[bufs.specs[n][0]]) + 4 * bufs.specs[n][3])
        setattr(g, n + "_bs", bufs.specs[n][1])
        setattr(g, n + "_cs", bufs.specs[n][2])
    _lib.check(_L().set_attention_bwd(C.byref(g), _s()), "set_attention_bwd")
    torch.cuda.synchronize()
    for n in ("x", "q", "k", "v", "kv", "do"):
        if n in cpu:
            assert torch.equal(dbuf[n].cpu(), cpu[n]), n
    same_bits = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert same_bits(dbuf["o"].cpu(), got_o) and same_bits(dbuf["lse"].cpu(), got_lse) and same_bits(dbuf["p"].cpu(), got_p)
    got = dbuf["delta"].cpu()
    _cmp(c["name"] + ".delta", tag, got, *_embed_want(got, lambda t: t[G:-G].view(B, heads, Tq), mo["delta"], bars["delta"]))
    done = set()
    for n in ("dq", "dk", "dv"):
        bname = bufs.specs[n][0]
        if bname in done:
            continue
        done.add(bname)
        members = [m_ for m_ in ("dq", "dk", "dv") if bufs.specs[m_][0] == bname]
        got = dbuf[bname].cpu()
        want = torch.full(got.shape, SENTINEL, dtype=torch.float64)
        bar = torch.zeros(got.shape, dtype=torch.float64)
        for m_ in members:
            bufs.view(want, m_).copy_(mo[m_])
            bufs.view(bar, m_).copy_(bars[m_])
        _cmp("%s.%s" % (c["name"], "+".join(members)), tag, got, want, bar, key=key(members[0]) if len(members) == 1 else None)
        if mode == "bounded":
            for m_ in members:
                gv, wv, bv = bufs.view(got, m_).double(), mo[m_], bars[m_]
                ok = torch.isfinite(wv) & (bv > 0)
                if bool(ok.any()):
                    WORST[(m_, dt)] = max(WORST.get((m_, dt), 0.0), float(((gv - wv).abs()[ok] / bv[ok]).max()))
    for b in dead_b.nonzero().flatten().tolist():
        gq, gk, gv = (bufs.view(dbuf[bufs.specs[n][0]].cpu(), n)[b] for n in ("dq", "dk", "dv"))
        assert bool((gq == 0).all()) and bool((gk == 0).all()) and bool(torch.isnan(gv).all())
    return o


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c,d", R.FUSED_RUNS, ids=R.FUSED_IDS)
def test_fused_attention_branch(dev, c, d, dt, mode):
    _run_fused(dev, c, d, mode, dt)


BOUNDED_DENSE = [(c, d) for c, d in R.FUSED_RUNS if c["layout"] != "strided"]


@pytest.mark.parametrize("c,d", BOUNDED_DENSE, ids=["%s-d%d" % (c["name"], d) for c, d in BOUNDED_DENSE])
def test_fused_and_composed_attention_side_by_side(dev, c, d):
    """The fused call and ops.attention_views (bmm -> softmax -> bmm) on the same bounded case, both against float64.  A report, not a
    verdict on either (both are code under test); what is asserted is only that both are NaN where float64 is."""
    from set_amd import ops
    o = R.make_fused(c["name"], d, "bounded")
    mo = o["want"]["f32"]
    H, MV = c["heads"] * d, ops.MatView
    if c["layout"] == "packed":
        x = torch.cat([o["q"], o["k"], o["v"]], 1).to(dev).contiguous()
        views = (MV.heads(x, c["heads"], 0, H), MV.heads(x, c["heads"], H, H), MV.heads(x, c["heads"], 2 * H, H))
    else:
        xq, xkv = o["q"].to(dev).contiguous(), torch.cat([o["k"], o["v"]], 1).to(dev).contiguous()
        views = (MV.heads(xq, c["heads"]), MV.heads(xkv, c["heads"], 0, H), MV.heads(xkv, c["heads"], H, H))
    kd = o["kpm"].to(dev) if o["kpm"] is not None else None
    assert ops._COMPUTE_DTYPE == "f32"
    of, _, pf = ops.attention_fused(*views, c["heads"], kd, c["fill"], o["alpha"], want_p=True)
    oc, pc = ops.attention_views(*views, c["heads"], kd, c["fill"], o["alpha"])
    torch.cuda.synchronize()
    err = {}
    for tag, go, gp in (("fused", of, pf), ("composed", oc, pc)):
        for n, gt in (("o", go), ("p", gp)):
            dlt = (gt.cpu().double() - mo[n]).abs()
            ok = torch.isfinite(mo[n])
            assert bool(torch.isnan(gt.cpu()[~ok]).all())
            err[tag, n] = float(dlt[ok].max()) if bool(ok.any()) else 0.0
    print("%s d%d: max err vs float64: o fused %.3e composed %.3e, p fused %.3e composed %.3e" % (
        c["name"], d, err["fused", "o"], err["composed", "o"], err["fused", "p"], err["composed", "p"]))


# ------------------------------------------------------------------------------------------------------------------------
# refusals: the documented code, every output untouched.  Every operand is valid and large enough for the call as if it were run
# ------------------------------------------------------------------------------------------------------------------------
def _small_call(dev, head_dim=32):
    from set_amd import _lib
    B, heads, Tq, Tk = 2, 2, 5, 8
    n = B * heads * 96 * 8 + 64  # room for head_dim up to 96
    ins = {k_: torch.ones(n, device=dev) for k_ in ("q", "k", "v", "do")}
    outs = {k_: torch.full((n,), SENTINEL, device=dev) for k_ in ("o", "lse", "delta", "dq", "dk", "dv")}
    g = _lib.SetAttnBwdArgs()
    a = g.fwd
    a.q, a.k, a.v, a.o, a.lse = _p(ins["q"]), _p(ins["k"]), _p(ins["v"]), _p(outs["o"]), _p(outs["lse"])
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = heads * head_dim * Tq, heads * head_dim * Tk, heads * head_dim * Tk, heads * head_dim * Tq
    a.q_cs, a.k_cs, a.v_cs, a.o_cs = Tq, Tk, Tk, Tq
    a.B, a.heads, a.head_dim, a.Tq, a.Tk = B, heads, head_dim, Tq, Tk
    a.scale, a.fill, a.bf16 = 0.25, R.NEG_INF, 0
    g.d_o, g.delta, g.dq, g.dk, g.dv = _p(ins["do"]), _p(outs["delta"]), _p(outs["dq"]), _p(outs["dk"]), _p(outs["dv"])
    g.dq_bs, g.dk_bs, g.dv_bs, g.dq_cs, g.dk_cs, g.dv_cs = a.q_bs, a.k_bs, a.v_bs, Tq, Tk, Tk
    return g, ins, outs


ATTN_REFUSED = [  # why, entry point, field (of fwd unless bwd-only), value, code
    ("null q", "fwd", "q", None, E_INVALID), ("null o", "fwd", "o", None, E_INVALID), ("null lse", "fwd", "lse", None, E_INVALID),
    ("Tq 0", "fwd", "Tq", 0, E_INVALID), ("head_dim 48", "fwd", "head_dim", 48, E_UNSUPPORTED),
    ("bwd: null q", "bwd", "q", None, E_INVALID), ("bwd: Tq 0", "bwd", "Tq", 0, E_INVALID), ("bwd: head_dim 48", "bwd", "head_dim", 48, E_UNSUPPORTED),
    ("bwd: null d_o", "bwd", "d_o", None, E_INVALID), ("bwd: null delta", "bwd", "delta", None, E_INVALID), ("bwd: null dq", "bwd", "dq", None, E_INVALID),
]


@pytest.mark.parametrize("why,entry,field,value,code", ATTN_REFUSED, ids=[r[0].replace(" ", "_").replace(":", "") for r in ATTN_REFUSED])
def test_attention_refuses_and_leaves_every_output_alone(dev, why, entry, field, value, code):
    g, ins, outs = _small_call(dev, 48 if field == "head_dim" else 32)
    if field == "head_dim":
        g.fwd.head_dim = 48
    else:
        setattr(g if field in ("d_o", "delta", "dq") else g.fwd, field, value)
    rc = _L().set_attention(C.byref(g.fwd), _s()) if entry == "fwd" else _L().set_attention_bwd(C.byref(g), _s())
    assert rc == code, why
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs.values()) and all(bool((t == 1.0).all()) for t in ins.values())


def test_attention_runs_the_call_the_refusals_are_variations_of(dev):
    g, ins, outs = _small_call(dev)
    assert _L().set_attention(C.byref(g.fwd), _s()) == 0 and _L().set_attention_bwd(C.byref(g), _s()) == 0
    torch.cuda.synchronize()
    n = 2 * 2 * 32 * 5
    assert bool((outs["o"][:n] == 1.0).all()) and bool((outs["o"][n:] == SENTINEL).all())  # the mean of ones
    assert bool((outs["dq"][:n] == 0.0).all()) and bool((outs["dq"][n:] == SENTINEL).all())  # equal keys: no gradient for q


# ------------------------------------------------------------------------------------------------------------------------
# set_bmm
# ------------------------------------------------------------------------------------------------------------------------
def _store(mat, how, rows_first):
    """[nb, R, Cc] -> flat storage and (row stride, col stride, batch stride) of the logical matrix in it."""
    nb, Rr, Cc = mat.shape
    if how == rows_first:               # as is: rows of Cc
        return mat.contiguous().flatten(), Cc, 1, Rr * Cc
    if how == "pad":                    # every other element of rows twice as long; BIG between
        st = torch.full((nb, Rr, 2 * Cc), BIG)
        st[:, :, ::2] = mat
        return st.flatten(), 2 * Cc, 2, Rr * 2 * Cc
    return mat.transpose(1, 2).contiguous().flatten(), 1, Rr, Rr * Cc  # transposed storage


def _bmm_call(dev, case, mode):
    from set_amd import _lib
    name, no, ni, M, N, K, sa, sb, _, acc, _ = case
    o = R.make_bmm(case, mode)
    nb = no * ni
    fa, a_ms, a_ks, a_b = _store(o["A"], sa, "mk")
    fb, b_ks, b_ns, b_b = _store(o["B"], sb, "kn")
    assert ((a_ms, a_ks), (b_ks, b_ns)) == R.bmm_strides(case)
    c_ms, c_bi = N + 3, M * (N + 3) + 5
    c_bo = ni * c_bi + 7
    off = 9
    cbuf = torch.full((off + (no - 1) * c_bo + (ni - 1) * c_bi + (M - 1) * c_ms + N + G,), SENTINEL)
    cview = lambda t: t.as_strided((no, ni, M, N), (c_bo, c_bi, c_ms, 1), off)
    if acc:
        cview(cbuf).copy_(o["C0"].view(no, ni, M, N))
    want, bar = torch.full(cbuf.shape, SENTINEL, dtype=torch.float64), torch.zeros(cbuf.shape, dtype=torch.float64)
    cview(want).copy_(o["want"].view(no, ni, M, N))
    cview(bar).copy_(o["bar"].view(no, ni, M, N))
    da, db, dc = fa.to(dev), fb.to(dev), cbuf.to(dev)
    g = _lib.SetBmmArgs()
    g.A, g.B, g.C = _p(da), _p(db), _p(dc) + 4 * off
    g.a_bo, g.a_bi, g.a_ms, g.a_ks = ni * a_b, a_b, a_ms, a_ks
    g.b_bo, g.b_bi, g.b_ks, g.b_ns = ni * b_b, b_b, b_ks, b_ns
    g.c_bo, g.c_bi, g.c_ms, g.c_ns = c_bo, c_bi, c_ms, 1
    g.n_outer, g.n_inner, g.M, g.N, g.K = no, ni, M, N, K
    g.alpha, g.accumulate = o["alpha"], int(acc)
    _lib.check(_L().set_bmm(C.byref(g), _s()), "set_bmm")
    torch.cuda.synchronize()
    assert torch.equal(da.cpu(), fa) and torch.equal(db.cpu(), fb)
    return dc.cpu(), want, bar


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("case", R.BMM, ids=[c[0] for c in R.BMM])
def test_bmm_branch(dev, case, mode):
    got, want, bar = _bmm_call(dev, case, mode)
    _cmp(case[0], "bmm " + mode, got, want, bar, key=("bmm", "f32") if mode == "bounded" else None)


def test_bmm_into_a_column_major_c_gives_the_bits_of_the_row_major_call(dev):
    """ops.bmm runs the transposed problem when c is column-major (c^T = b^T a^T): the same products in the same k order."""
    from set_amd import ops
    g = torch.Generator().manual_seed(5)
    no, ni, M, N, K = 2, 3, 70, 45, 50
    nb = no * ni
    A, Bm = torch.randn(nb, M, K, generator=g).to(dev), torch.randn(nb, K, N, generator=g).to(dev)
    MV = ops.MatView
    av, bv = MV(A, no, ni, M, K, ni * M * K, M * K, K, 1), MV(Bm, no, ni, K, N, ni * K * N, K * N, N, 1)
    c_row, c_col = torch.full((nb, M, N), SENTINEL, device=dev), torch.full((nb, N, M), SENTINEL, device=dev)
    ops.bmm(av, bv, MV(c_row, no, ni, M, N, ni * M * N, M * N, N, 1), alpha=0.3)
    cv = MV(c_col, no, ni, M, N, ni * M * N, M * N, 1, M)
    assert cv.rs == 1 and cv.cs != 1
    ops.bmm(av, bv, cv, alpha=0.3)
    torch.cuda.synchronize()
    assert torch.equal(c_col.transpose(1, 2), c_row)
    ref = 0.3 * (A.double() @ Bm.double())
    assert float((c_row.double() - ref).abs().max()) <= float(((K + 2) * R.U * 0.3 * (A.abs().double() @ Bm.abs().double()) + 2 * R.U * ref.abs()).max())


def test_bmm_and_positions_refusals(dev):
    from set_amd import _lib
    n = 65536
    a, b = torch.ones(n, device=dev), torch.ones(n, device=dev)
    c = torch.full((n + 64,), SENTINEL, device=dev)
    g = _lib.SetBmmArgs()
    g.A, g.B, g.C = _p(a), _p(b), _p(c)
    g.a_bo = g.b_bo = g.c_bo = g.a_bi = g.b_bi = g.c_bi = 1
    g.a_ms = g.a_ks = g.b_ks = g.b_ns = g.c_ms = g.c_ns = 1
    g.n_outer, g.n_inner, g.M, g.N, g.K, g.alpha, g.accumulate = n, 1, 1, 1, 1, 1.0, 0
    assert _L().set_bmm(C.byref(g), _s()) == E_INVALID       # a batch above 65535 (the grid's z limit)
    g.n_outer, g.K = 4, 0
    assert _L().set_bmm(C.byref(g), _s()) == E_INVALID       # K = 0
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all())
    g.K = 1
    assert _L().set_bmm(C.byref(g), _s()) == 0               # the call they are variations of
    torch.cuda.synchronize()
    assert bool((c[:4] == 1.0).all()) and bool((c[4:] == SENTINEL).all())
    tok, x = torch.ones(2, 8, dtype=torch.int64, device=dev), torch.ones(2, 8, device=dev)
    pos = torch.full((2 * 8 + 64,), int(SENTINEL), dtype=torch.int64, device=dev)
    assert _L().set_make_positions(_p(tok), _p(x), 8, _p(pos), 2, 8, _s()) == E_INVALID    # both inputs
    assert _L().set_make_positions(None, None, 8, _p(pos), 2, 8, _s()) == E_INVALID        # neither
    torch.cuda.synchronize()
    assert bool((pos == int(SENTINEL)).all())


# ------------------------------------------------------------------------------------------------------------------------
# the small kernels
# ------------------------------------------------------------------------------------------------------------------------
def _guarded(dev, n, dtype=torch.float32, fill=SENTINEL):
    buf = torch.full((G + n + G,), fill, dtype=dtype, device=dev)
    return buf, _p(buf) + G * buf.element_size()


def _guards_intact(buf, fill=SENTINEL):
    return bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("case", R.SOFTMAX, ids=["r%d_c%d" % c[:2] for c in R.SOFTMAX])
def test_softmax_rows_forward_and_backward(dev, case, mode):
    from set_amd import _lib
    rows, cols, rpb, masked, fill = case
    o = R.make_softmax(case, mode)
    xd = o["x"].to(dev)
    kd = o["kpm"].to(dev) if o["kpm"] is not None else None
    buf, ptr = _guarded(dev, rows * cols)
    _lib.check(_L().set_softmax_rows(_p(xd), _p(kd), ptr, rows, cols, rpb, fill, _s()), "set_softmax_rows")
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), o["x"]) and _guards_intact(buf)
    _cmp("softmax r%d c%d" % (rows, cols), mode, buf[G:-G].cpu().view(rows, cols), o["p"], o["bar_p"], key=("softmax", "f32") if mode == "bounded" else None)
    pd, dpd = o["pf"].to(dev), o["dp"].to(dev)
    buf, ptr = _guarded(dev, rows * cols)
    _lib.check(_L().set_softmax_rows_bwd(_p(pd), _p(dpd), ptr, rows, cols, _s()), "set_softmax_rows_bwd")
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu(), o["pf"]) and torch.equal(dpd.cpu(), o["dp"]) and _guards_intact(buf)
    _cmp("softmax bwd r%d c%d" % (rows, cols), mode, buf[G:-G].cpu().view(rows, cols), o["ds"], o["bar_ds"])


@pytest.mark.parametrize("source", ["tokens", "x"])
@pytest.mark.parametrize("T", R.POSITIONS_T)
def test_make_positions(dev, T, source):
    from set_amd import _lib
    B = 4
    tok = R.make_tokens(B, T, T)
    want = R.positions_ref(tok != 0)
    buf, ptr = _guarded(dev, B * T, torch.int64, int(SENTINEL))
    if source == "tokens":
        td = tok.to(dev)
        _lib.check(_L().set_make_positions(_p(td), None, 0, ptr, B, T, _s()), "set_make_positions")
    else:  # channel 0 of a [B][3][T] tensor; 0.5 and -1 count, -0.0 does not; the other channels hold what must not be read
        x = torch.full((B, 3, T), 1.0)
        vals = torch.tensor([0.5, -1.0, 2.0])
        x[:, 0] = torch.where(tok != 0, vals[tok % 3], torch.tensor([0.0, -0.0])[torch.arange(T) % 2].expand(B, T))
        x[:, 1:] = torch.where(tok != 0, 0.0, 1.0)[:, None, :]
        xd = x.to(dev)
        _lib.check(_L().set_make_positions(None, _p(xd), 3 * T, ptr, B, T, _s()), "set_make_positions")
    torch.cuda.synchronize()
    assert _guards_intact(buf, int(SENTINEL)) and torch.equal(buf[G:-G].cpu().view(B, T), want)


@pytest.mark.parametrize("B,heads,n", R.HEAD_MEAN)
def test_head_mean(dev, B, heads, n):
    from set_amd import _lib
    g = torch.Generator().manual_seed(n)
    p = torch.randint(-8, 9, (B, heads, n), generator=g).float()
    buf, ptr = _guarded(dev, B * n)
    pd = p.to(dev)
    _lib.check(_L().set_head_mean(_p(pd), ptr, B, heads, n, _s()), "set_head_mean")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and torch.equal(buf[G:-G].cpu().view(B, n).double(), p.double().mean(1)) and torch.equal(pd.cpu(), p)


@pytest.mark.parametrize("B,Cc,T", R.MASK_FILL)
def test_mask_fill_chan(dev, B, Cc, T):
    from set_amd import _lib
    g = torch.Generator().manual_seed(B * Cc * T)
    x, e = torch.randint(-5, 6, (B, Cc, T), generator=g).float(), torch.randint(-5, 6, (Cc,), generator=g).float()
    m = (torch.rand(B, T, generator=g) < 0.4).float()
    want = x.double() * (1 - m.double()[:, None]) + e.double()[None, :, None] * m.double()[:, None]
    buf, ptr = _guarded(dev, B * Cc * T)
    _lib.check(_L().set_mask_fill_chan(_p(x.to(dev)), _p(e.to(dev)), _p(m.to(dev)), ptr, B, Cc, T, _s()), "set_mask_fill_chan")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and torch.equal(buf[G:-G].cpu().view(B, Cc, T).double(), want)


@pytest.mark.parametrize("mode", ["exact", "bounded"])
@pytest.mark.parametrize("B,Cc,T", R.CHANNEL_SUM)
def test_masked_channel_sum_adds_to_what_is_there(dev, B, Cc, T, mode):
    from set_amd import _lib
    g = torch.Generator().manual_seed(B * Cc * T + (mode == "exact"))
    if mode == "exact":
        d_, out0 = torch.randint(-5, 6, (B, Cc, T), generator=g).float(), torch.randint(-9, 10, (Cc,), generator=g).float()
    else:
        d_, out0 = torch.randn(B, Cc, T, generator=g), torch.randn(Cc, generator=g)
    m = (torch.rand(B, T, generator=g) < 0.4).float()
    terms = d_.double() * m.double()[:, None]
    want = out0.double() + terms.sum((0, 2))
    # per thread ceil(B T / 256) adds, six exchanges, three adds across the waves, the add to out
    bar = torch.zeros(Cc, dtype=torch.float64) if mode == "exact" else (math.ceil(B * T / 256) + 10) * R.U * (terms.abs().sum((0, 2)) + out0.abs().double())
    buf, ptr = _guarded(dev, Cc)
    buf[G:-G] = out0.to(dev)
    dd, md = d_.to(dev), m.to(dev)
    _lib.check(_L().set_masked_channel_sum(_p(dd), _p(md), ptr, B, Cc, T, _s()), "set_masked_channel_sum")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and torch.equal(dd.cpu(), d_)
    _cmp("channel sum %d %d %d" % (B, Cc, T), mode, buf[G:-G].cpu(), want, bar)


def test_zz_report_worst_fraction_of_the_bar():
    """Not a check: prints, per output and operand type, the worst |d| / bar the bounded cases of this run reached."""
    for key_ in sorted(WORST):
        print("worst fraction of the bar: %-8s %-5s %.3f" % (key_[0], key_[1], WORST[key_]))
