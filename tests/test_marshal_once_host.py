"""CPU: every libhsp entry-point family is marshalled at ONE call site of the package, and the bf16 working-copy registry forgets a
``Bf16Params`` that has died.

A family is the literal head of ``_run``'s first argument -- a string, the left end of a ``+`` chain, the head of an f-string, either
arm of a conditional --, so ``"hsp_gather_max_bwd" + sfx`` and ``"hsp_gather_max_bwd_sel" + sfx`` are two families and a suffix
choice stays inside its wrapper.  A function that passes one of its own parameters on as that head (``_rf_bwd_dirs_call``'s ``base``
and ``base + "_partial"``) is no site itself: the calls that hand it a literal are.

The same walk holds the two layer nodes to ONE conv2 + ORL tail each way (every wrapper of that tail is called from one function
body of ops.py), and "fold this weight gradient now" and "pad a thin gradient to 64 columns" to one statement each, in ops.py."""
import ast
import gc
import glob
import os
import weakref

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hs_pose_amd")

# functions whose one ``_run`` site takes the entry's name from its caller, each a single site by construction
EXEMPT = {
    "_compact": 'f"hsp_{name}": one site that serves the three compaction entries',
    "_label_boxes": 'f"hsp_{name}": one site that serves the label-box entries (per frame / per tracked instance)',
    "_to_pcl": 'f"hsp_{name}": one site that serves the back-projection entries (shared / per-item depth frame)',
    "_wgrad_custom": "the family (hsp_wgrad / hsp_wgrad_ragged) is the dispatch's own answer, handed in as ``entry``; its two calls are "
                     "the direct and the _partial entry of that one family",
}
DELETED_ALIASES = ("hs_layer", "_wgrad", "_orl_fwd", "_colsum", "_rf_conv_fwd", "_rf_conv_bwd")


def _heads(node):
    """the literal heads an expression can start with, or None where it does not start with a literal"""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return {node.value}
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
        return _heads(node.left)
    if isinstance(node, ast.JoinedStr) and node.values:
        return _heads(node.values[0])
    if isinstance(node, ast.IfExp):
        a, b = _heads(node.body), _heads(node.orelse)
        return None if a is None or b is None else a | b
    return None


def _leftmost_name(node):
    while isinstance(node, ast.BinOp):
        node = node.left
    return node.id if isinstance(node, ast.Name) else None


def _callee(call):
    f = call.func
    return f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None


def _calls_by_function(tree):
    """(enclosing function or None, Call) for every call of a module"""
    out = []

    def walk(node, fn):
        for child in ast.iter_child_nodes(node):
            inner = child if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else fn
            if isinstance(child, ast.Call):
                out.append((fn, child))
            walk(child, inner)
    walk(tree, None)
    return out


def _sites():
    """({family: [where, ...]}, [unresolved where, ...]) over the package"""
    trees = {os.path.basename(p): ast.parse(open(p).read()) for p in sorted(glob.glob(os.path.join(PKG, "*.py")))}
    calls = [(f, fn, c) for f, t in trees.items() for fn, c in _calls_by_function(t)]
    sites, unresolved, forwarders = {}, [], {}          # forwarders: function name -> index of the parameter it passes on
    for f, fn, c in calls:
        if _callee(c) != "_run" or not c.args or (fn and fn.name in EXEMPT):
            continue
        where = f"{f}:{c.lineno} ({fn.name if fn else 'module'})"
        heads = _heads(c.args[0])
        if heads is not None:
            for h in heads:
                sites.setdefault(h, []).append(where)
            continue
        name = _leftmost_name(c.args[0])
        params = [a.arg for a in fn.args.args] if fn else []
        if name in params:
            forwarders[fn.name] = params.index(name) - (1 if params[0] in ("self", "cls") else 0)
        else:
            unresolved.append(where)
    for f, fn, c in calls:
        at = forwarders.get(_callee(c))
        if at is None or len(c.args) <= at:
            continue
        where = f"{f}:{c.lineno} ({fn.name if fn else 'module'})"
        heads = _heads(c.args[at])
        if heads is None:
            unresolved.append(where)
        for h in heads or ():
            sites.setdefault(h, []).append(where)
    return sites, unresolved


def test_each_family_has_one_call_site():
    sites, unresolved = _sites()
    assert len(sites) > 100                                    # (the walk found the package's calls)
    assert not unresolved, f"_run with a name no literal heads, outside the listed exemptions: {unresolved}"
    twice = {fam: where for fam, where in sites.items() if len(where) != 1}
    assert not twice, "marshalled at more than one call site:\n" + "\n".join(f"  {k}: {v}" for k, v in sorted(twice.items()))


def test_pooling_backward_families_stay_apart():
    sites, _ = _sites()
    for fam in ("hsp_gather_max_bwd", "hsp_gather_max_bwd_sel", "hsp_gather_max_bwd_csr", "hsp_gather_max_fwd", "hsp_gather_max_fwd_sel",
                "hsp_pool_fwd", "hsp_pool_fwd_sel", "hsp_gather_rows_bwd", "hsp_gather_rows_bwd_csr", "hsp_rf_surface_fwd",
                "hsp_rf_surface_bwd", "hsp_split_params_x3"):
        assert len(sites.get(fam, ())) == 1, (fam, sites.get(fam))


def test_ops_bf16_holds_no_batchnorm_entry_and_no_alias():
    tree = ast.parse(open(os.path.join(PKG, "ops_bf16.py")).read())
    strings = [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
    assert not [s for s in strings if "hsp_bn_" in s]
    top = set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            top.add(node.name)
        elif isinstance(node, ast.Assign):
            top |= {n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)}
    assert not top & set(DELETED_ALIASES)


# ---- the layer nodes' shared tails, "fold now", "thin pad" ----------------------------------------------------------------------

# the wrappers of the conv2 + ORL tail: each is called from one function body of ops.py (the forward or the backward tail)
TAIL_WRAPPERS = ("_orl_fwd_exact", "_orl_fwd_counts_raw", "_layer_out_exact", "_layer_out_rows", "_orl_bwd_small", "_orl_bwd_accumulate_raw")


def _tree(name):
    return ast.parse(open(os.path.join(PKG, name)).read())


def _body(fn):
    """one function BODY: its name with the line of its ``def`` (two classes' ``forward`` are two bodies), or 'module'"""
    return f"{fn.name}:{fn.lineno}" if fn else "module"


def _bare_wgrad_assigners(tree, skip_classes=()):
    """the function bodies (or 'module') that assign to an attribute ``bare_wgrad``, outside the classes listed"""
    out = set()

    def walk(node, fn):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef) and child.name in skip_classes:
                continue
            inner = child if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else fn
            if isinstance(child, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
                targets = child.targets if isinstance(child, ast.Assign) else [child.target]
                if any(isinstance(n, ast.Attribute) and n.attr == "bare_wgrad" for t in targets for n in ast.walk(t)):
                    out.add(_body(fn))
            walk(child, inner)
    walk(tree, None)
    return out


def _tail_callers(tree):
    """{wrapper: the function bodies that call it}"""
    callers = {name: set() for name in TAIL_WRAPPERS}
    for fn, c in _calls_by_function(tree):
        if _callee(c) in callers:
            callers[_callee(c)].add(_body(fn))
    return callers


def test_each_tail_wrapper_is_called_from_one_function():
    assert not {k: sorted(v) for k, v in _tail_callers(_tree("ops.py")).items() if len(v) != 1}


def test_the_walk_tells_two_methods_of_one_name_apart():
    """the nodes' methods share their names: a wrapper called from two classes' ``forward``, or a save and restore of
    ``bare_wgrad`` in two classes' ``backward``, is two bodies"""
    two = ast.parse("class A:\n    def forward(s):\n        _orl_fwd_exact()\n        sf.bare_wgrad = 0\n"
                    "class B:\n    def forward(s):\n        _orl_fwd_exact()\n        sf.bare_wgrad = 0\n")
    assert len(_tail_callers(two)["_orl_fwd_exact"]) == 2 and len(_bare_wgrad_assigners(two)) == 2


def test_fold_now_is_stated_once():
    assert len(_bare_wgrad_assigners(_tree("ops.py"), skip_classes=("StepFolds", "WgradBatch"))) == 1
    assert not _bare_wgrad_assigners(_tree("ops_bf16.py"))


def test_ops_bf16_pads_no_thin_gradient():
    pads = [c.lineno for _, c in _calls_by_function(_tree("ops_bf16.py"))
            if _callee(c) in ("zeros", "new_zeros") and any(isinstance(a, ast.Constant) and a.value == 64 for a in c.args)]
    assert not pads


# ---- ops._copies ---------------------------------------------------------------------------------------------------------------

def test_copies_leave_with_their_bf16params():
    from hs_pose_amd import ops, ops_bf16
    from hs_pose_amd._lib import HspError
    a, b = torch.randn(8, 16), torch.randn(4, 8)
    reg = ops_bf16.Bf16Params([(a, True, True), (b, True, False)])          # (lays out copies and a table: launches nothing)
    assert a.data_ptr() in ops._copies and b.data_ptr() in ops._copies
    c, ct = ops.copies_of(a)
    assert tuple(c.shape) == (8, 16) and tuple(ct.shape) == (16, 8) and ops.copies_of(b)[1] is None
    del reg, c, ct
    gc.collect()
    assert a.data_ptr() not in ops._copies and b.data_ptr() not in ops._copies
    # the tensor the registry was built over, kept alive apart from it: the very address and shape a re-used block would have
    for t in (a, b, torch.randn(8, 16)):
        with pytest.raises(HspError, match="no bf16 working copy registered"):
            ops.copies_of(t)


def test_copies_of_ignores_an_entry_whose_owner_is_dead():
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError

    class Owner:
        pass
    a, owner = torch.randn(8, 16), Owner()
    entry = (torch.empty(8, 16, dtype=torch.bfloat16), torch.empty(16, 8, dtype=torch.bfloat16), weakref.ref(owner))
    ops._copies[a.data_ptr()] = entry
    try:
        assert ops.copies_of(a)[0] is entry[0]
        del owner
        gc.collect()
        with pytest.raises(HspError, match="no bf16 working copy registered"):
            ops.copies_of(a)
    finally:
        ops._copies.pop(a.data_ptr(), None)
