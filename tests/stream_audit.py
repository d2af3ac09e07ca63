"""Leaf-stream audit: a recorder for the library calls of a training step and a checker for the rules of leaf_stream.py.

The leaf stream (set_amd/leaf_stream.py, autograd_ops._leaves) is correct only while five rules hold that no numeric test can see: a race
between the two streams almost never changes a bit.  They are checkable on the host, from the ORDER of the library calls and their
pointer arguments:

  R1 held      every pointer a leaf-stream call reads lies in a view held by the stream's OperandLedger at that moment, or in a
               long-lived buffer the test names (the flat optimizer's buffers) or the leaf stream's own scratch pool entries
  R2 no alloc  the caching allocator's allocation counter does not move inside a block, except for a scratch regrow whose old buffer
               went to hold_until_join and whose new buffer is the pool entry
  R3 writers   every pointer a leaf-stream call writes lies in the flat gradient buffer inside a .grad view the optimizer handed out
               (FlatAdamW.sink) since the previous block, or in the leaf stream's scratch
  R4 conflict  while a leaf call is pending (until a join, or the completed marker that covers its block) no compute-stream library
               call writes into an extent it reads or touches an extent it writes
  R5 release   release_upto(n) only after set_stream_mark_done returned 1 for a marker recorded after the last leaf call of what is
               released and covering exactly n; no slot re-recorded while outstanding; release_all only right after a join
  R6 join      a join precedes set_adamw, set_sumsq_det on the flat gradient and the successful return of backward(); a bucket
               all-reduce launched while leaf work is pending goes through leaf_fence's fork

Three parts: `header_roles()` parses include/set_amd.h into (argument, read / write) tables; `Recorder` is a proxy over the loaded
library plus wrappers of the leaf-stream bookkeeping that appends plain dicts to one list; `check()` is a pure function of that list
(no torch device, no library), so every rule is tested on the CPU with hand-written logs.  ATen kernels do not pass through the proxy:
R4 sees the project's own launches only; the starved-stream test of test_gpu_stream_audit.py covers the rest.
"""
import ast
import collections
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "set_amd.h")
AUTOGRAD_OPS = os.path.join(ROOT, "speech-editing-toolkit_amd", "autograd_ops.py")

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. roles from the header
# ---------------------------------------------------------------------------------------------------------------------------------
Param = collections.namedtuple("Param", "name ctype pointer const struct")  # struct: name of the args struct a pointer points to, or None


def _strip_comments(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _decls(text, structs):
    """`const float *a, *b` / `int64_t n` / `SetAttnArgs fwd` -> [Param]; one C declaration without its semicolon."""
    text = " ".join(text.split())
    if not text:
        return []
    m = re.match(r"^((?:const\s+)?(?:unsigned\s+)?\w+(?:\s+const)?)\s*(.*)$", text)
    base, rest = m.group(1), m.group(2)
    const = "const" in base.split()
    btype = " ".join(w for w in base.split() if w != "const")
    out = []
    for d in rest.split(","):
        d = d.strip()
        stars = d.count("*")
        name = d.replace("*", "").replace("const", "").strip()
        name = re.sub(r"\[.*\]$", "", name)
        out.append(Param(name, btype, stars > 0, const, btype if btype in structs else None))
    return out


def parse_header(path=HEADER):
    """(functions, structs): functions[name] = [Param] in declaration order, structs[name] = [Param] (fields, nested structs kept as
    one non-pointer field whose .struct names them)."""
    src = _strip_comments(open(path).read())
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        name, body = m.group(3), m.group(2)
        fields = []
        for decl in body.split(";"):
            fields += _decls(decl, structs)
        structs[name] = fields
    src = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", src, flags=re.S)
    functions = {}
    for m in re.finditer(r"\b(set_\w+)\s*\(([^()]*)\)\s*;", src):
        name, args = m.group(1), m.group(2).strip()
        params = []
        if args and args != "void":
            for a in args.split(","):
                params += _decls(a, structs)
        functions[name] = params
    return functions, structs


def struct_pointer_fields(structs, name, prefix=""):
    """[(dotted field path, 'r' | 'w')] of the pointer fields of an args struct, nested structs flattened."""
    out = []
    for f in structs[name]:
        if f.pointer:
            out.append((prefix + CTYPES_FIELD.get(f.name, f.name), "r" if f.const else "w"))
        elif f.struct:
            out += struct_pointer_fields(structs, f.struct, prefix + f.name + ".")
    return out


# Pointers that name a stream or host memory, not a device operand: (entry point, argument).  `void *stream` (always the last argument)
# is the launch stream of every entry point and is handled by name.
STREAM_ARGS = {("set_stream_order", "first"), ("set_stream_order", "after"), ("set_stream_mark", "stream")}
HOST_POINTER_ARGS = {
    ("set_stream_create_low_priority", "out"): "the new stream handle is written to host memory",
    ("set_conv_x2_range_flag", "flag"): "host int32 read-back",
    ("set_selftest_mfma", "max_err_host"): "host float read-back",
    ("set_stft_geometries", "triples"): "host table",
    ("set_stft_sizes", "out8"): "host table",
    ("set_fill_pack_desc", "d"): "host descriptor filled for a later upload",
}

# Where the header's qualifier says less than the kernels do: (args struct, field) -> (role, why).  SetAttnBwdArgs embeds the forward's
# SetAttnArgs, whose outputs are inputs of the backward.
ROLE_OVERRIDES = {
    ("SetAttnBwdArgs", "fwd.o"): ("r", "attention_fused.hip: attn_bwd_dq_kernel only loads o (delta = sum dO * O); the dK/dV pass does not touch it"),
    ("SetAttnBwdArgs", "fwd.lse"): ("r", "attention_fused.hip: both backward passes read the saved row max / sum through const pointers"),
    ("SetAttnBwdArgs", "fwd.p"): ("r", "set_amd.h: fwd.p is unused by set_attention_bwd"),
}
DEVICE_STRUCT_ARRAYS = {("set_pack_conv_weights_batch", "descs_dev")}  # a device array of descriptors: an operand, not an args struct
CTYPES_FIELD = {"in": "inp"}  # header field -> ctypes field where the header's name is a Python keyword

# Integer-address arguments: the call sites build these from saved addresses (C.c_void_p(ptr), struct fields assigned .data_ptr()
# integers, `dd.data_ptr() + ...`), so no tensor stands behind the value the proxy sees.  Their roles are stated here by hand and
# test_stream_audit_reference.py holds them against the header's const qualifiers.
INT_ADDRESS_ROLES = {
    ("set_conv1d_wgrad", "dw"): "w", ("set_conv1d_wgrad_det", "dw"): "w",          # conv_wgrad(dw_ptr=...): a row slice of a packed weight's .grad
    ("set_conv1d_wgrad_det_grouped", "dw"): "w",                                    # conv_wgrad_grouped(dw_ptr): layer 0's .grad view
    ("set_step_proj_bwd_dw", "dw"): "w", ("set_step_proj_bwd_dw", "db"): "w",      # _grouped_targets base pointers
    ("set_diffnet_layers_bwd_reduce", "db_out"): "w", ("set_diffnet_layers_bwd_reduce", "db_dil"): "w",
    ("set_diffnet_layers_bwd_reduce", "db_cond"): "w",
    ("set_diffnet_layer_bwd_reduce", "dd"): "w",                                    # dd.data_ptr() + 4 l C: a column block of dd
    ("SetDiffnetLayerBf16BwdArgs", "dy16"): "w", ("SetDiffnetLayerBf16BwdArgs", "do16"): "w", ("SetDiffnetLayerBf16BwdArgs", "y16"): "r",
    ("SetDiffnetLayerBf16BwdArgs", "dx_out"): "r", ("SetDiffnetLayerBf16BwdArgs", "dx"): "w", ("SetDiffnetLayerBf16BwdArgs", "img"): "r",
    ("SetDiffnetLayerBf16BwdArgs", "part_dbo"): "w", ("SetDiffnetLayerBf16BwdArgs", "part_dby"): "w",
    ("SetDiffnetLayerBf16BwdArgs", "part_dd"): "w",
    ("SetDiffnetLayerBf16Args", "x_in"): "r", ("SetDiffnetLayerBf16Args", "x_out"): "w", ("SetDiffnetLayerBf16Args", "dstep"): "r",
    ("SetDiffnetLayerBf16Args", "y16"): "w", ("SetDiffnetLayerBf16Args", "z16"): "w",
    ("SetDiffnetStackArgs", "dstep"): "r",                                          # ops.diffnet_stack(dmat.data_ptr(), ...)
}


def header_roles(path=HEADER):
    """{entry point: [(position, argument, kind, role, struct)]} for every pointer argument; kind is 'dev' (device operand), 'stream',
    'host' or 'args' (pointer to an args struct, whose fields are in struct_roles); role 'r' for const, 'w' otherwise.
    Returns (roles, struct_roles) with struct_roles[struct] = [(dotted field, role)]."""
    functions, structs = parse_header(path)
    roles = {}
    for name, params in functions.items():
        rows = []
        for i, p in enumerate(params):
            if not p.pointer:
                continue
            role = "r" if p.const else "w"
            if p.struct and (name, p.name) not in HOST_POINTER_ARGS and (name, p.name) not in DEVICE_STRUCT_ARRAYS:
                kind = "args"
            elif p.name == "stream" and i == len(params) - 1 or (name, p.name) in STREAM_ARGS:
                kind = "stream"
            elif (name, p.name) in HOST_POINTER_ARGS:
                kind = "host"
            else:
                kind = "dev"
            rows.append((i, p.name, kind, role, p.struct))
        roles[name] = rows
    struct_roles = {s: [(path, ROLE_OVERRIDES.get((s, path), (role,))[0]) for path, role in struct_pointer_fields(structs, s)] for s in structs}
    return roles, struct_roles


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the call sites of autograd_ops.py
# ---------------------------------------------------------------------------------------------------------------------------------
SITE_CALLS = ("_leaves", "_conv_leaves", "leaf_work")


def leaf_sites(path=AUTOGRAD_OPS, source=None):
    """Every `_leaves(` / `_conv_leaves(` / `leaf_work(` call of autograd_ops.py (or of `source`) in line order:
    [(site id "Class.function#k:callee", first line, last line)]; k counts the sites of one function."""
    tree = ast.parse(open(path).read() if source is None else source)
    found = []

    def walk(node, scope):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.ClassDef, ast.FunctionDef)):
                walk(child, scope + [child.name])
            else:
                if isinstance(child, ast.Call):
                    callee = child.func.attr if isinstance(child.func, ast.Attribute) else getattr(child.func, "id", None)
                    if callee in SITE_CALLS:
                        found.append((".".join(scope), callee, child.lineno, child.end_lineno))
                walk(child, scope)

    walk(tree, [])
    found.sort(key=lambda r: r[2])
    count, out = collections.Counter(), []
    for scope, callee, a, b in found:
        out.append(("%s#%d:%s" % (scope, count[scope], callee), a, b))
        count[scope] += 1
    return out


# Which audited GPU case (test_gpu_stream_audit.CASES) reaches each site.  A site added to autograd_ops.py has no entry here and fails
# test_stream_audit_reference.py until a case that reaches it is named; the GPU test then demands that the case did reach it.
WRAPPER = "wrapper"  # not a case: the two leaf_work( calls inside _leaves itself, which every other site goes through (the frame of
#                      _leaves has returned by the time the block is entered, so the recorder cannot see it on the stack)
SITE_CASES = {
    "_leaves#0:leaf_work": WRAPPER,
    "_leaves#1:leaf_work": WRAPPER,
    "_conv_leaves#0:_leaves": "spec_f32_per_op",
    "_Conv1dFn.backward#0:_conv_leaves": "spec_f32_per_op",
    "_PreLnFfnFn.backward#0:_conv_leaves": "campnet_fused",
    "_PreLnFfnFn.backward#1:_conv_leaves": "campnet_fused",
    "_StutterLossFn.backward#0:_leaves": "stutter",
    "_EmbeddingFn.backward#0:_leaves": "spec_f32_stack",
    "_DiffNetStackFn.backward#0:_leaves": "spec_f32_stack",
    "_bf16_stack_bwd_grouped#0:_leaves": "spec_bf16_grouped",
    "_StepProjFn.backward#0:_leaves": "spec_f32_stack",
    "_PreLnSelfAttnFn.backward#0:_conv_leaves": "campnet_fused",
    "_PreLnSelfAttnFn.backward#1:_conv_leaves": "campnet_fused",
    "_PreLnCrossAttnFn.backward#0:_conv_leaves": "campnet_fused",
    "_PreLnCrossAttnFn.backward#1:_leaves": "campnet_fused",
}
CASE_NAMES = ("spec_f32_stack", "spec_f32_per_op", "spec_bf16_grouped", "stutter", "campnet_fused", "campnet_per_op")


def unmapped_sites(sites, table=None):
    """Sites without a case, and table entries without a site."""
    table = SITE_CASES if table is None else table
    ids = [s for s, _a, _b in sites]
    return [s for s in ids if s not in table], [s for s in table if s not in ids]


def site_of_frames(frames, sites):
    """The audited call sites on a stack: frames = [(file name, line)] innermost first; returns the site ids, innermost first."""
    out = []
    for fname, line in frames:
        if os.path.basename(fname) != "autograd_ops.py":
            continue
        hits = [s for s, a, b in sites if a <= line <= b]
        out += hits
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. what the leaf-callable entry points touch, from their own shape arguments (all of them take flat arguments, no args struct)
# ---------------------------------------------------------------------------------------------------------------------------------
def _named(fn_params, args):
    return {p.name: a for p, a in zip(fn_params, args)}


def _ext_wgrad(a):
    return {"dw": [(a["dw"], 4 * a["Cout"] * a["Cin"] * a["K"])]}


def _ext_wgrad_det(a):
    return {"dw": [(a["dw"], 4 * a["Cout"] * a["Cin"] * a["K"])], "scratch": [(a["scratch"], 4 * a["scratch_floats"])]}


def _ext_wgrad_grouped(a):
    n = 4 * a["Cout"] * a["Cin"] * a["K"]
    return {"dw": [(a["dw"] + 4 * q * a["dw_gs"], n) for q in range(a["groups"])], "scratch": [(a["scratch"], 4 * a["scratch_floats"])]}


def _ext_channel_sum(a):
    return {"out": [(a["out"], 4 * a["C"])], "scratch": [(a["scratch"], 4 * (2048 + a["C"]))]}  # channel_sum_ asks for 2048 + C floats


def _ext_scatter(a):
    return {"table": [(a["table"], 4 * a["n_rows"] * a["C"])], "scratch": [(a["scratch"], 4)]}


def _ext_step_proj_dw(a):
    return {"dw": [(a["dw"] + 4 * q * a["dw_ls"], 4 * a["C"] * a["C"]) for q in range(a["L"])],
            "db": [(a["db"] + 4 * q * a["db_ls"], 4 * a["C"]) for q in range(a["L"])]}


def _ext_stutter_reduce(a):
    return {"dw": [(a["dw"], 4 * 3 * a["C"])], "db": [(a["db"], 4 * 3)]}


LEAF_WRITE_EXTENTS = {
    "set_conv1d_wgrad": _ext_wgrad,
    "set_conv1d_wgrad_det": _ext_wgrad_det,
    "set_conv1d_wgrad_det_grouped": _ext_wgrad_grouped,
    "set_channel_sum_det": _ext_channel_sum,
    "set_scatter_rows_det": _ext_scatter,
    "set_step_proj_bwd_dw": _ext_step_proj_dw,
    "set_stutter_head_bwd_reduce": _ext_stutter_reduce,
}


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the recorder
# ---------------------------------------------------------------------------------------------------------------------------------
def _addr(v):
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    if isinstance(v, C.c_void_p):
        return v.value or 0
    if hasattr(v, "value"):
        return v.value or 0
    return 0


def view_extent(t):
    """(data_ptr, bytes spanned) of a tensor view."""
    if t.numel() == 0:
        return (t.data_ptr(), 0)
    span = 1 + sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride()))
    return (t.data_ptr(), span * t.element_size())


def _tensors(obj, out):
    import torch
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _tensors(o, out)
    return out


class _Proxy:
    """Stands in for the loaded library (set_amd._lib._lib): forwards every call, logs those that carry a stream or a pointer."""

    def __init__(self, real, rec):
        self.__dict__["_real"], self.__dict__["_rec"], self.__dict__["_cache"] = real, rec, {}

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            real = getattr(self._real, name)
            fn = self._rec._wrap_call(name, real) if name in self._rec.roles else real
            self._cache[name] = fn
        return fn


class Recorder:
    def __init__(self):
        self.roles, self.struct_roles = header_roles()
        self.functions, _ = parse_header()
        self.sites = leaf_sites()
        self.events = []
        self.sites_reached = collections.Counter()

    # ---- library calls
    def _wrap_call(self, name, real):
        rows = self.roles[name]
        params = self.functions[name]
        if not rows and not name.startswith("set_stream_"):
            return real
        events, ext_fn = self.events, LEAF_WRITE_EXTENTS.get(name)

        def call(*args):
            from set_amd import ops
            stream, ptrs = None, []
            for i, arg, kind, role, struct in rows:
                v = args[i]
                if kind == "stream":
                    if arg in ("stream",):
                        stream = _addr(v)
                elif kind == "dev":
                    a = _addr(v)
                    if a:
                        ptrs.append((arg, role, a, None))
                elif kind == "args":
                    obj = getattr(v, "_obj", v)
                    obj = obj.contents if hasattr(obj, "contents") else obj
                    for path, frole in self.struct_roles[struct]:
                        o = obj
                        for part in path.split("."):
                            o = getattr(o, part)
                        a = _addr(o)
                        if a:
                            ptrs.append((path, frole, a, None))
            ev = {"k": "call", "name": name, "stream": stream, "leaf": getattr(ops._STREAM_TLS, "leaf", None) is not None, "ptrs": ptrs}
            if name.startswith("set_stream_"):
                ev["args"] = [_addr(a) if not isinstance(a, int) else a for a in args if not hasattr(a, "_obj")]
            if ev["leaf"] and ext_fn is not None:  # a leaf call: the extents it writes, from its own shape arguments
                named = {p.name: (_addr(a) if p.pointer else a) for p, a in zip(params, args)}
                sized = ext_fn(named)
                ev["ptrs"] = [p for p in ptrs if p[0] not in sized] + [(arg, "w", a, n) for arg, ex in sized.items() for a, n in ex if a]
            events.append(ev)
            ret = real(*args)
            ev["ret"] = ret
            return ret

        return call

    # ---- the bookkeeping around them
    def _scratch_snapshot(self, st):
        from set_amd import autograd_ops as A
        out = {}
        for pool_name, pool in (("det", A._DET_SCRATCH), ("wg", A._WG_SCRATCH)):
            for (dev, stream), buf in pool.items():
                if stream == st.raw.value:
                    out[pool_name] = (buf.data_ptr(), buf.numel() * buf.element_size())
        return out

    def install(self, monkeypatch):
        import torch
        from set_amd import _lib, leaf_stream, parallel, training
        rec, events = self, self.events
        monkeypatch.setattr(_lib, "_lib", _Proxy(_lib.lib(), self))
        LW, LS, OL = leaf_stream.leaf_work, leaf_stream.LeafStream, leaf_stream.OperandLedger

        def alloc_count():
            return torch.cuda.memory_stats()["allocation.all.allocated"]

        enter0, exit0 = LW.__enter__, LW.__exit__

        def enter(self_):
            events.append({"k": "enter_begin"})
            on = enter0(self_)
            ev = {"k": "enter", "on": bool(on)}
            if on:
                frames, f = [], sys._getframe(1)
                while f is not None and len(frames) < 12:
                    frames.append((f.f_code.co_filename, f.f_lineno))
                    f = f.f_back
                ev["sites"] = site_of_frames(frames, rec.sites)
                for s in ev["sites"]:
                    rec.sites_reached[s] += 1
                ev["leaf_stream"] = self_._st.raw.value
                ev["scratch"] = rec._scratch_snapshot(self_._st)
                ev["alloc"] = alloc_count()
            events.append(ev)
            return on

        def exit_(self_, *exc):
            if self_.on:
                events.append({"k": "exit", "alloc": alloc_count(), "scratch": rec._scratch_snapshot(self_._st), "exc": exc[0] is not None})
            else:
                events.append({"k": "exit", "off": True})
            return exit0(self_, *exc)

        monkeypatch.setattr(LW, "__enter__", enter)
        monkeypatch.setattr(LW, "__exit__", exit_)

        def logged(cls, meth, make):
            orig = getattr(cls, meth)

            def wrapper(self_, *a):
                ev = make(self_, *a)
                events.append(ev)
                ret = orig(self_, *a)
                ev["ret"] = ret if isinstance(ret, (int, type(None))) else None
                return ret

            monkeypatch.setattr(cls, meth, wrapper)

        for meth in ("fork", "join", "mark", "poll", "release_all"):
            logged(LS, meth, lambda st, _m=meth: {"k": "ls_" + _m, "raw": st.raw.value})

        hold0 = OL.hold

        def hold(self_, obj):
            hold0(self_, obj)
            ts = _tensors(obj, [])
            events.append({"k": "hold", "n": self_.count, "views": [view_extent(t) for t in ts],
                           "storages": [(t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()) for t in ts], "bytes": self_.bytes})

        monkeypatch.setattr(OL, "hold", hold)
        logged(OL, "release_upto", lambda led, n: {"k": "release_upto", "n": n})
        logged(OL, "release_all", lambda led: {"k": "release_all"})

        huj0 = leaf_stream.hold_until_join

        def hold_until_join(buf):
            events.append({"k": "hold_until_join", "ptr": buf.data_ptr(), "bytes": buf.numel() * buf.element_size()})
            return huj0(buf)

        monkeypatch.setattr(leaf_stream, "hold_until_join", hold_until_join)

        from set_amd import autograd_ops as A, ops

        def scratch_logged(pool_name, pool, orig):
            def scratch(device, n_floats):
                key = (device, ops._stream().value)
                old = pool.get(key)
                buf = orig(device, n_floats)
                if buf is not old:
                    events.append({"k": "scratch_new", "pool": pool_name, "stream": key[1], "ptr": buf.data_ptr(),
                                   "bytes": buf.numel() * buf.element_size(), "old": None if old is None else old.data_ptr()})
                return buf
            return scratch

        monkeypatch.setattr(A, "_det_scratch", scratch_logged("det", A._DET_SCRATCH, A._det_scratch))
        monkeypatch.setattr(A, "_wg_scratch", scratch_logged("wg", A._WG_SCRATCH, A._wg_scratch))

        sink0 = training.FlatAdamW.sink

        def sink(self_, param):
            g = sink0(self_, param)
            if g is not None:
                events.append({"k": "sink", "ptr": g.data_ptr(), "bytes": g.numel() * g.element_size()})
            return g

        monkeypatch.setattr(training.FlatAdamW, "sink", sink)

        launch0 = parallel.GradBucketer._launch

        def launch(self_, b, why):
            events.append({"k": "bucket_begin", "bucket": b})
            try:
                return launch0(self_, b, why)
            finally:
                events.append({"k": "bucket_end", "bucket": b})

        monkeypatch.setattr(parallel.GradBucketer, "_launch", launch)

        backward0 = torch.Tensor.backward

        def backward(self_, *a, **kw):
            events.append({"k": "backward_begin"})
            try:
                ret = backward0(self_, *a, **kw)
            except BaseException:
                events.append({"k": "backward_end", "ok": False})
                raise
            events.append({"k": "backward_end", "ok": True})
            return ret

        monkeypatch.setattr(torch.Tensor, "backward", backward)
        return self


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the checker: a pure function of the event list
# ---------------------------------------------------------------------------------------------------------------------------------
Violation = collections.namedtuple("Violation", "rule index name why")


def _inside(addr, ext):
    return ext[0] <= addr < ext[0] + max(ext[1], 1)


def _overlap(a, b):
    return a[0] < b[0] + max(b[1], 1) and b[0] < a[0] + max(a[1], 1)


def check(events, long_lived=(), flat_grad=None):
    """[Violation] of the rules R1-R6 in `events`.  long_lived: [(ptr, bytes, reason)] buffers that outlive every step (the test names
    them one by one); flat_grad: (ptr, bytes) of the optimizer's flat gradient buffer."""
    out = []
    long_lived = [(p, n) for p, n, _why in long_lived]
    # the leaf stream's scratch of every block: what the pools held at its enter or its exit
    block_scratch, cur = {}, None
    for i, ev in enumerate(events):
        if ev["k"] == "enter" and ev.get("on"):
            cur = i
            block_scratch[cur] = list(ev.get("scratch", {}).values())
        elif ev["k"] == "scratch_new" and cur is not None and ev["stream"] == events[cur].get("leaf_stream"):
            block_scratch[cur].append((ev["ptr"], ev["bytes"]))
        elif ev["k"] == "exit" and not ev.get("off") and cur is not None:
            block_scratch[cur] += list(ev.get("scratch", {}).values())
            cur = None

    leaf_raw = None          # raw handle of the leaf stream
    holds = []               # (n, [view extents]) currently in the ledger
    n_held = 0               # count of the last hold
    block = None             # index of the open block's enter event
    block_n = 0              # the ledger's count once the open block's operands were held: the number a marker must cover
    enter_ev = None
    sinks = []               # .grad views handed out since the previous block's exit
    huj = []                 # buffers given to hold_until_join inside the open block
    regrown = []             # (pool, new buffer) of the scratch regrows inside the open block whose old buffer was held (or did not exist)
    pending = []             # leaf calls not yet known to have run: (index, name, block_n, read extents, write extents)
    joined_at = -1           # index of the last join with no leaf call after it
    marks = {}               # slot -> (index of its set_stream_mark, count it covers) while outstanding
    done = []                # (slot, index, covers) of markers seen complete and not yet consumed by a release_upto
    last_leaf_call_of = {}   # block_n -> index of its last leaf call
    in_bucket = None

    for i, ev in enumerate(events):
        k = ev["k"]
        if k == "enter" and ev.get("on"):
            block, enter_ev, block_n, huj, regrown = i, ev, n_held, [], []
            leaf_raw = ev.get("leaf_stream", leaf_raw)
        elif k == "exit" and not ev.get("off"):
            if block is not None and enter_ev is not None and "alloc" in ev and "alloc" in enter_ev:
                delta = ev["alloc"] - enter_ev["alloc"]
                entry = dict(enter_ev.get("scratch", {}))
                for pool, ptr_bytes in regrown:   # the regrown buffers are the pool entries the block leaves behind
                    entry[pool] = ptr_bytes
                if delta != len(regrown) or entry != ev.get("scratch", {}):
                    out.append(Violation("R2", i, "exit", "%d allocation(s) inside the block, %d explained by a scratch regrow whose old buffer "
                                         "was held and whose new buffer is the pool entry" % (delta, len(regrown))))
            block, enter_ev, sinks = None, None, []
        elif k == "hold":
            n_held = ev["n"]
            holds.append((ev["n"], list(ev["views"])))
        elif k == "hold_until_join":
            huj.append(ev["ptr"])
        elif k == "scratch_new":
            if block is not None and ev["stream"] == leaf_raw and (ev["old"] is None or ev["old"] in huj):
                regrown.append((ev["pool"], (ev["ptr"], ev["bytes"])))
        elif k == "sink":
            sinks.append((ev["ptr"], ev["bytes"]))
        elif k == "release_upto":
            n = ev["n"]
            hit = [d for d in done if d[2] == n]
            if not hit:
                out.append(Violation("R5", i, "release_upto", "release_upto(%d) without a completed marker that covers %d" % (n, n)))
            else:
                slot, mark_index, _ = hit[0]
                done.remove(hit[0])
                late = [j for bn, j in last_leaf_call_of.items() if bn <= n and j > mark_index]
                if late:
                    out.append(Violation("R5", i, "release_upto", "the marker (event %d) was recorded before leaf call %d of what it releases"
                                         % (mark_index, late[0])))
            holds = [h for h in holds if h[0] > n]
            pending = [p for p in pending if p[2] > n]
        elif k == "release_all":
            if joined_at < 0:
                out.append(Violation("R5", i, "release_all", "release_all without a join right before it"))
            holds, pending, marks, done = [], [], {}, []
        elif k == "bucket_begin":
            in_bucket = {"index": i, "pending": bool(pending), "fork": False}
        elif k == "bucket_end":
            if in_bucket and in_bucket["pending"] and not in_bucket["fork"]:
                out.append(Violation("R6", in_bucket["index"], "bucket all-reduce", "launched with leaf work pending and no leaf_fence fork"))
            in_bucket = None
        elif k == "backward_end":
            if ev.get("ok") and pending:
                out.append(Violation("R6", i, "backward", "backward() returned with %d leaf call(s) not joined" % len(pending)))
        elif k == "call":
            name, stream = ev["name"], ev.get("stream")
            if name == "set_stream_order":
                src, dst = ev["args"][0], ev["args"][1]
                if leaf_raw is not None and src == leaf_raw:      # join: the current stream waits for the leaf stream
                    pending, joined_at = [], i
                elif in_bucket is not None and (leaf_raw is None or dst == leaf_raw):
                    in_bucket["fork"] = True
                continue
            if name == "set_stream_mark":
                slot = ev["args"][1]
                if slot in marks:
                    out.append(Violation("R5", i, name, "slot %d recorded again while its marker is outstanding" % slot))
                marks[slot] = (i, n_held)
                continue
            if name == "set_stream_mark_done":
                slot = ev["args"][0]
                if ev.get("ret") == 1 and slot in marks:
                    done.append((slot,) + marks.pop(slot))
                continue
            if name.startswith("set_stream_"):
                continue
            is_leaf = leaf_raw is not None and stream == leaf_raw
            if is_leaf:
                joined_at = -1
                if name not in LEAF_WRITE_EXTENTS:
                    out.append(Violation("R3", i, name, "a leaf-stream entry point without a rule for what it writes"))
                scratch = block_scratch.get(block, [])
                held = [v for _, views in holds for v in views]
                reads, writes = [], []
                for arg, role, addr, nbytes in ev["ptrs"]:
                    if role == "r":
                        home = [e for e in held if _inside(addr, e)]
                        if home:  # what the call may read: its own extent where its shape arguments give one, else the whole held view
                            reads.append((addr, nbytes) if nbytes else home[0])
                        elif not any(_inside(addr, e) for e in long_lived + scratch):
                            out.append(Violation("R1", i, name, "reads %s = %#x, which no held operand, long-lived buffer or leaf scratch contains"
                                                 % (arg, addr)))
                    else:
                        ext = (addr, nbytes or 1)
                        writes.append(ext)
                        in_scratch = any(_inside(addr, e) and addr + ext[1] <= e[0] + e[1] for e in scratch)
                        in_sink = (flat_grad is not None and _inside(addr, flat_grad)
                                   and any(_inside(addr, s) and addr + ext[1] <= s[0] + s[1] for s in sinks))
                        if not (in_scratch or in_sink):
                            out.append(Violation("R3", i, name, "writes %s = %#x (+%d bytes): neither a .grad view handed to this node nor the "
                                                 "leaf stream's scratch" % (arg, addr, ext[1])))
                pending.append((i, name, block_n, reads, writes))
                last_leaf_call_of[block_n] = i
            else:
                for arg, role, addr, nbytes in ev["ptrs"]:
                    ext = (addr, nbytes or 1)
                    for j, lname, _bn, reads, writes in pending:
                        if role == "w" and any(_overlap(ext, r) for r in reads):
                            out.append(Violation("R4", i, name, "writes %s = %#x inside an operand that pending leaf call %d (%s) reads"
                                                 % (arg, addr, j, lname)))
                        if any(_overlap(ext, w) for w in writes):
                            out.append(Violation("R4", i, name, "touches %s = %#x inside what pending leaf call %d (%s) writes" % (arg, addr, j, lname)))
                if name == "set_adamw" and pending:
                    out.append(Violation("R6", i, name, "the optimizer runs with %d leaf call(s) not joined" % len(pending)))
                if name == "set_sumsq_det" and pending and flat_grad is not None and any(_inside(a, flat_grad) for _, r, a, _n in ev["ptrs"] if r == "r"):
                    out.append(Violation("R6", i, name, "the gradient norm reads the flat gradient with %d leaf call(s) not joined" % len(pending)))
    return out


def stats(events):
    """Counts for profiles/stream_audit.log."""
    leaf_raw, blocks, calls, names, peak, marker_rel, early, inside_enter = None, 0, 0, set(), 0, 0, 0, False
    for ev in events:
        k = ev["k"]
        if k == "enter_begin":
            inside_enter = True
        elif k == "enter":
            inside_enter = False
            if ev.get("on"):
                blocks += 1
                leaf_raw = ev["leaf_stream"]
        elif k == "hold":
            peak = max(peak, ev.get("bytes", 0))
        elif k == "release_upto":
            marker_rel += 1 if ev.get("ret") else 0
        elif k == "ls_join" and inside_enter:
            early += 1
        elif k == "call" and leaf_raw is not None and ev.get("stream") == leaf_raw and not ev["name"].startswith("set_stream_"):
            calls += 1
            names.add(ev["name"])
    return {"blocks": blocks, "leaf_calls": calls, "leaf_entry_points": sorted(names), "peak_held_bytes": peak,
            "marker_releases": marker_rel, "early_joins": early}
