"""The leaf-stream audit itself (tests/stream_audit.py), without a GPU: the header parse against the ctypes binding, every rule of the
checker against a hand-written log with one planted violation, and the inventory of the leaf call sites of autograd_ops.py."""
import copy
import ctypes as C

import pytest

import stream_audit as S

CUR, LEAF = 0x1000, 0x9000                       # raw stream handles
FLAT_G = (0x100000, 4096)                        # the flat gradient buffer
LONG = [(0x200000, 4096, "flat parameters"), (FLAT_G[0], FLAT_G[1], "flat gradients")]
G, X, G2, X2 = (0x2000, 1024), (0x3000, 512), (0x4000, 1024), (0x5000, 512)   # operands
SCR = (0x8000, 4096)                             # the leaf stream's wgrad scratch


def call(name, stream, ptrs=(), leaf=False, args=None, ret=0):
    ev = {"k": "call", "name": name, "stream": stream, "leaf": leaf, "ptrs": [tuple(p) for p in ptrs], "ret": ret}
    if args is not None:
        ev["args"] = list(args)
    return ev


def fork():
    return call("set_stream_order", None, args=[CUR, LEAF, 0])


def join():
    return call("set_stream_order", None, args=[LEAF, CUR, 1])


def block(n, views, sink, alloc, pre=()):
    """One leaf block: [enter_begin, *pre, fork, hold, enter, the wgrad call, exit]."""
    return [{"k": "sink", "ptr": sink[0], "bytes": sink[1]},
            {"k": "enter_begin"}, *pre, fork(),
            {"k": "hold", "n": n, "views": list(views), "storages": list(views), "bytes": 0},
            {"k": "enter", "on": True, "leaf_stream": LEAF, "scratch": {"wg": SCR}, "alloc": alloc, "sites": []},
            call("set_conv1d_wgrad_det", LEAF, [("g", "r", views[0][0], None), ("x", "r", views[1][0] + 64, None),
                                                ("dw", "w", sink[0], sink[1]), ("scratch", "w", SCR[0], 1024)], leaf=True),
            {"k": "exit", "alloc": alloc, "scratch": {"wg": SCR}, "exc": False}]


def clean_log():
    """Two blocks of one backward pass: the first one's operands are released by its marker at the second one's entry, the pass ends
    with the join, then the gradient norm and the optimizer."""
    ev = [{"k": "backward_begin"}]
    ev += block(1, [G, X], (FLAT_G[0], 256), 10)
    ev += [call("set_stream_mark", LEAF, args=[LEAF, 0, 0]),
           call("set_act_bwd", CUR, [("z", "r", G[0], None), ("dy", "r", X[0], None), ("dz", "w", 0x6000, None)])]
    ev += block(2, [G2, X2], (FLAT_G[0] + 256, 256), 12,
                pre=[call("set_stream_mark_done", None, args=[0], ret=1), {"k": "release_upto", "n": 1, "ret": 1}])
    ev += [call("set_stream_mark", LEAF, args=[LEAF, 1, 0]),
           join(), {"k": "release_all"}, {"k": "backward_end", "ok": True},
           call("set_sumsq_det", CUR, [("g", "r", FLAT_G[0], None), ("out", "w", 0x7000, None)]),
           call("set_adamw", CUR, [("p", "w", 0x200000, None), ("g", "r", FLAT_G[0], None)])]
    return ev


def find(ev, pred, nth=0):
    return [i for i, e in enumerate(ev) if pred(e)][nth]


def is_call(name):
    return lambda e: e["k"] == "call" and e["name"] == name


def rules(ev):
    return [(v.rule, v.index) for v in S.check(ev, LONG, FLAT_G)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the header parse
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binding():
    import set_amd  # noqa: F401
    from set_amd import _lib
    return _lib


def _is_pointer_type(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_header_parse_finds_every_entry_point_and_its_pointers(binding):
    functions, _ = S.parse_header()
    roles, struct_roles = S.header_roles()
    assert sorted(binding.SIGNATURES) == sorted(functions)
    for name, (_res, argtypes) in binding.SIGNATURES.items():
        assert len(functions[name]) == len(argtypes), name
        rows = roles[name]
        assert [i for i, *_ in rows] == [i for i, t in enumerate(argtypes) if _is_pointer_type(t)], name
        for i, arg, kind, role, struct in rows:
            t = argtypes[i]
            if kind == "args":       # a pointer to an args struct: the binding declares the same structure
                assert t._type_.__name__ == struct, (name, arg)
            elif kind == "host":     # host memory: never a bare address in the binding
                assert t is not C.c_void_p or (name, arg) in S.HOST_POINTER_ARGS, (name, arg)
            else:
                assert t is C.c_void_p, (name, arg, kind)
        # the launch stream is the trailing `void *stream`, and never an operand
        streams = [arg for _i, arg, kind, *_ in rows if kind == "stream"]
        if functions[name] and functions[name][-1].name == "stream":
            assert streams == ["stream"], name
    named = {(n, r[1]) for n, rows in roles.items() for r in rows}
    assert all(key in named for table in (S.HOST_POINTER_ARGS, S.STREAM_ARGS, S.DEVICE_STRUCT_ARRAYS) for key in table)
    assert all(path in [f for f, _r in S.struct_pointer_fields(S.parse_header()[1], s)] for s, path in S.ROLE_OVERRIDES)


def test_struct_fields_match_the_ctypes_structures(binding):
    _, structs = S.parse_header()
    _, struct_roles = S.header_roles()
    seen = 0
    for name, cls in vars(binding).items():
        if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure:
            seen += 1
            want = [S.CTYPES_FIELD.get(f.name, f.name) for f in structs[name]]
            assert want == [f[0] for f in cls._fields_], name
            for f, (fname, ftype) in zip(structs[name], cls._fields_):
                assert f.pointer == _is_pointer_type(ftype), (name, fname)
            obj = cls()
            for path, role in struct_roles[name]:   # every pointer field the recorder will read exists on the structure
                o = obj
                for part in path.split("."):
                    o = getattr(o, part)
                assert role in "rw"
    assert seen == len(structs) >= 15
    assert ("fwd.q", "r") in struct_roles["SetAttnBwdArgs"] and ("dq", "w") in struct_roles["SetAttnBwdArgs"]


def test_integer_address_roles_agree_with_the_header():
    roles, struct_roles = S.header_roles()
    for (owner, arg), role in S.INT_ADDRESS_ROLES.items():
        if owner in struct_roles:
            assert (arg, role) in struct_roles[owner], (owner, arg)
        else:
            assert [r[3] for r in roles[owner] if r[1] == arg and r[2] == "dev"] == [role], (owner, arg)


def test_leaf_callable_entry_points_take_flat_arguments():
    """What a leaf block launches (wgrad, channel sum, scatter, step-projection dW, stutter reduce): no args struct, so the extents they
    write follow from their own scalar arguments."""
    functions, _ = S.parse_header()
    roles, _ = S.header_roles()
    for name, ext in S.LEAF_WRITE_EXTENTS.items():
        assert all(kind != "args" for _i, _a, kind, *_ in roles[name]), name
        args = {p.name: (0x10000 * (i + 1) if p.pointer else 3) for i, p in enumerate(functions[name])}
        sized = ext(args)
        written = {a for _i, a, kind, role, _s in roles[name] if kind == "dev" and role == "w"}
        assert set(sized) == written, (name, sized, written)   # a size for every pointer the entry point writes
        assert all(n > 0 for ex in sized.values() for _a, n in ex)
    g = S.LEAF_WRITE_EXTENTS["set_conv1d_wgrad_det_grouped"]({"dw": 1000, "groups": 3, "dw_gs": 50, "Cout": 2, "Cin": 3, "K": 1,
                                                              "scratch": 9000, "scratch_floats": 7})
    assert g["dw"] == [(1000, 24), (1200, 24), (1400, 24)] and g["scratch"] == [(9000, 28)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------------------
def test_clean_log_passes():
    assert S.check(clean_log(), LONG, FLAT_G) == []
    st = S.stats(clean_log())
    assert st["blocks"] == 2 and st["leaf_calls"] == 2 and st["leaf_entry_points"] == ["set_conv1d_wgrad_det"] and st["marker_releases"] == 1


def test_r1_a_read_outside_every_held_operand_is_flagged():
    ev = clean_log()
    i = find(ev, is_call("set_conv1d_wgrad_det"), 1)
    ev[i]["ptrs"][1] = ("x", "r", X[0], None)   # the FIRST block's x: released by the marker before this call
    assert rules(ev) == [("R1", i)]
    ev = clean_log()
    i = find(ev, is_call("set_conv1d_wgrad_det"))
    ev[i]["ptrs"][0] = ("g", "r", 0x200000 + 8, None)   # a long-lived buffer the test names: allowed
    assert rules(ev) == []
    ev[i]["ptrs"][0] = ("g", "r", 0x300000, None)       # alive or not: not held, not named
    assert rules(ev) == [("R1", i)]


def test_r2_an_allocation_inside_a_block_is_flagged_and_a_held_scratch_regrow_is_not():
    ev = clean_log()
    i = find(ev, lambda e: e["k"] == "exit")
    ev[i]["alloc"] += 1
    assert rules(ev) == [("R2", i)]

    def regrow(ev, held):
        """The first block's kernel needs a larger scratch: the pool entry is replaced inside the block."""
        new = (0xA000, 8192)
        c = find(ev, is_call("set_conv1d_wgrad_det"))
        ev[c]["ptrs"][3] = ("scratch", "w", new[0], 8192)
        ev[c:c] = ([{"k": "hold_until_join", "ptr": SCR[0], "bytes": SCR[1]}] if held else []) + [
            {"k": "scratch_new", "pool": "wg", "stream": LEAF, "ptr": new[0], "bytes": new[1], "old": SCR[0]}]
        x = find(ev, lambda e: e["k"] == "exit")
        ev[x]["alloc"] += 1
        for e in ev[x:]:
            if e["k"] in ("enter", "exit") and "scratch" in e:
                e["scratch"] = {"wg": new}
        ev[find(ev, is_call("set_conv1d_wgrad_det"), 1)]["ptrs"][3] = ("scratch", "w", new[0], 1024)
        return x

    ev = clean_log()
    regrow(ev, held=True)
    assert rules(ev) == []
    ev = clean_log()
    x = regrow(ev, held=False)   # kernels queued on the leaf stream may still use the old buffer: it has to go to hold_until_join
    assert rules(ev) == [("R2", x)]
    ev = clean_log()
    x = regrow(ev, held=True)
    ev[x]["scratch"] = {"wg": SCR}   # ... and the new buffer has to be the pool entry
    assert ("R2", x) in rules(ev)


def test_r3_a_leaf_write_outside_the_nodes_grad_views_is_flagged():
    ev = clean_log()
    i = find(ev, is_call("set_conv1d_wgrad_det"))
    ev[i]["ptrs"][2] = ("dw", "w", 0x6800, 256)                # a temporary
    assert rules(ev) == [("R3", i)]
    ev = clean_log()
    i = find(ev, is_call("set_conv1d_wgrad_det"), 1)
    ev[i]["ptrs"][2] = ("dw", "w", FLAT_G[0], 256)             # in the flat buffer, but the first block's parameter
    assert rules(ev) == [("R3", i)]
    ev = clean_log()
    ev[i]["ptrs"][2] = ("dw", "w", FLAT_G[0] + 256, 512)       # runs past the end of the view it was given
    assert rules(ev) == [("R3", i)]
    ev = clean_log()
    ev[find(ev, is_call("set_conv1d_wgrad_det"))]["name"] = "set_row_sum"   # an entry point the audit has no write rule for
    assert ("R3", find(ev, is_call("set_row_sum"))) in rules(ev)


def test_r4_a_compute_stream_write_into_a_pending_operand_is_flagged():
    ev = clean_log()
    i = find(ev, is_call("set_act_bwd"))
    ev[i]["ptrs"][2] = ("dz", "w", G[0] + 16, None)            # in place into the held gradient buffer
    assert rules(ev) == [("R4", i)]
    ev = clean_log()
    ev[i]["ptrs"][1] = ("dy", "r", FLAT_G[0] + 8, None)        # reads the .grad view the pending wgrad accumulates into
    assert rules(ev) == [("R4", i)]
    ev = clean_log()
    ev[i]["ptrs"][2] = ("dz", "w", G[0] + 16, None)
    k = find(ev, is_call("set_stream_mark_done"))              # the same write after the marker released the operand: no conflict
    ev.insert(k + 2, ev.pop(i))
    assert rules(ev) == []
    ev = clean_log()
    ev[i]["ptrs"][2] = ("dz", "w", X[0] + 256, 64)      # another slice of the held buffer, disjoint by the call's own extent ...
    assert rules(ev) == [("R4", i)]                            # ... is still inside the VIEW the leaf call may read
    j = find(ev, is_call("set_conv1d_wgrad_det"))
    ev[j]["ptrs"][1] = ("x", "r", X[0] + 64, 128)              # unless the leaf call's own shape arguments bound what it reads
    assert rules(ev) == []


def test_r5_releases_need_a_completed_marker_that_covers_them():
    ev = clean_log()
    ev[find(ev, is_call("set_stream_mark_done"))]["ret"] = 0   # polled, not complete
    i = find(ev, lambda e: e["k"] == "release_upto")
    assert rules(ev) == [("R5", i)]
    ev = clean_log()
    ev[i]["n"] = 2                                              # more than the marker covers
    assert ("R5", i) in rules(ev)
    ev = clean_log()                                            # the marker recorded BEFORE the block's kernel was launched
    m = find(ev, is_call("set_stream_mark"))
    ev.insert(find(ev, is_call("set_conv1d_wgrad_det")), ev.pop(m))
    assert rules(ev) == [("R5", i)]
    ev = clean_log()                                            # slot 0 recorded again while outstanding
    k = find(ev, is_call("set_stream_mark"), 1)
    ev[k]["args"][1] = 0
    ev[find(ev, is_call("set_stream_mark_done"))]["ret"] = 0
    del ev[i]
    assert rules(ev) == [("R5", k - 1)]
    ev = clean_log()                                            # release_all with leaf work after the last join
    r = find(ev, lambda e: e["k"] == "release_all")
    del ev[r - 1]
    assert ("R5", r - 1) in rules(ev)


def test_r6_readers_need_a_join():
    ev = clean_log()
    j = find(ev, lambda e: e["k"] == "call" and e["name"] == "set_stream_order" and e["args"][0] == LEAF)
    del ev[j:j + 2]                                             # no join at the end of backward(), none before the optimizer
    got = rules(ev)
    assert got == [("R6", find(ev, lambda e: e["k"] == "backward_end")), ("R6", find(ev, is_call("set_sumsq_det"))),
                   ("R6", find(ev, is_call("set_adamw")))]
    ev = clean_log()
    ev[find(ev, lambda e: e["k"] == "backward_end")]["ok"] = False   # a pass that raised returns without its join ...
    del ev[j:j + 2]
    ev.insert(find(ev, is_call("set_sumsq_det")), join())            # ... abort_step() / step() join before any reader
    assert rules(ev) == []
    # bucket all-reduce: through leaf_fence's fork while leaf work is pending
    ev = clean_log()
    k = find(ev, is_call("set_act_bwd"))
    ev[k:k] = [{"k": "bucket_begin", "bucket": 0}, {"k": "bucket_end", "bucket": 0}]
    assert rules(ev) == [("R6", k)]
    ev.insert(k + 1, fork())
    assert rules(ev) == []
    ev = clean_log()
    ev += [{"k": "bucket_begin", "bucket": 0}, {"k": "bucket_end", "bucket": 0}]   # nothing pending: no fence needed
    assert rules(ev) == []


def test_check_does_not_modify_the_log():
    ev = clean_log()
    before = copy.deepcopy(ev)
    S.check(ev, LONG, FLAT_G)
    assert ev == before


# ---------------------------------------------------------------------------------------------------------------------------------
# the call sites
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_leaf_call_site_maps_to_a_gpu_case():
    sites = S.leaf_sites()
    assert S.unmapped_sites(sites) == ([], [])
    ids = [s for s, _a, _b in sites]
    assert len(ids) == len(set(ids))
    # 12 sites in backward nodes + the one inside _conv_leaves + the two leaf_work( calls of the wrapper
    assert sum(1 for s in ids if s.endswith((":_leaves", ":_conv_leaves")) and not s.startswith("_conv_leaves#")) == 12
    assert [s for s in ids if s.endswith(":leaf_work")] == ["_leaves#0:leaf_work", "_leaves#1:leaf_work"]
    assert set(S.SITE_CASES.values()) <= set(S.CASE_NAMES) | {S.WRAPPER}
    assert all((v == S.WRAPPER) == k.startswith("_leaves#") for k, v in S.SITE_CASES.items())


def test_inventory_fails_for_a_site_without_a_case():
    src = open(S.AUTOGRAD_OPS).read() + '''

class _NewFusedFn(torch.autograd.Function):
    @staticmethod
    def backward(ctx, dy):
        with _leaves(dy.device, (None,), dy):
            pass
        r = _conv_leaves(dy, dy, None, None, None, None,
                         1, 1, 1, 1, 1, 0, 1, 1)
'''
    sites = S.leaf_sites(source=src)
    missing, stale = S.unmapped_sites(sites)
    assert missing == ["_NewFusedFn.backward#0:_leaves", "_NewFusedFn.backward#1:_conv_leaves"] and stale == []
    a, b = [(x, y) for s, x, y in sites if s == "_NewFusedFn.backward#1:_conv_leaves"][0]
    assert b == a + 1   # a call over two lines: either line of a frame finds it
    assert S.site_of_frames([("/x/autograd_ops.py", b), ("/x/other.py", b)], sites) == ["_NewFusedFn.backward#1:_conv_leaves"]
    table = dict(S.SITE_CASES)
    table["_Gone.backward#0:_leaves"] = "stutter"
    assert S.unmapped_sites(S.leaf_sites(), table) == ([], ["_Gone.backward#0:_leaves"])
