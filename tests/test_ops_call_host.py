"""CPU tests of the one path from Python into the HIP library: `ops._marshal` (what crosses the boundary), `ops._query`
against the built library, and the structure of tps_pp_amd/ops.py and optim.py -- `_lib.lib` and `_lib.check` are touched
only by `_call`, `_query` and the functions listed here with their reasons, so that a new wrapper cannot launch without
the device guard, on a stream of its own choosing or under a mistyped error label."""
import ast
import ctypes
import os

import torch

from tps_pp_amd import build, ops

PKG = os.path.dirname(os.path.abspath(ops.__file__))

# function or Class.method -> why it reaches the library without `_call` / `_query`
ALLOWED = {
    "ops.py": {
        "warp": "launches the pre-marshalled argument tuple of _warp_call, which WarpPlan takes as it is",
        "WarpPlan.__init__": "tpspp_warp_plan_create ends in the handle's address, not in a stream; keeps the run functions",
        "WarpPlan.run": "the headline's hot path: one foreign call on a stored handle, the status read only when non-zero",
        "conv2d_route": "host-side query of a host array whose negative result is an error code for _lib.check",
        "conv2d_bf16_route": "host-side query of pointers (alignment only) whose negative result is an error code for _lib.check",
        "nrtr_decoder_route": "host-side query of a host pointer table whose negative result is an error code",
        "warp_backward_route": "host-side query of pointers (alignment only) whose non-zero status is an error for _lib.check",
        "crnn_lstm_plan": "host-side query (through _query) whose negative result is an error code for _lib.check",
        "set_warp_bwd_accumulator": "process-wide setter: no tensor, no stream, no device",
        "set_warp_tuning": "process-wide setter: no tensor, no stream, no device",
    },
    "optim.py": {},
}


def _library_users(path):
    """Qualified names of the innermost functions of the file at `path` that reference `_lib.lib` or `_lib.check`."""
    users = set()

    def visit(node, scope, in_function):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                visit(child, scope + [child.name], True)
            elif isinstance(child, ast.ClassDef):
                visit(child, scope + [child.name], False)
            else:
                if isinstance(child, ast.Attribute) and child.attr in ("lib", "check") \
                        and isinstance(child.value, ast.Name) and child.value.id == "_lib":
                    users.add(".".join(scope) if in_function else "<module>")
                visit(child, scope, in_function)

    with open(path) as f:
        visit(ast.parse(f.read()), [], False)
    return users


def test_marshal_turns_tensors_into_pointers_and_nothing_else():
    t = torch.arange(6, dtype=torch.float32)
    arr = (ctypes.c_int * 3)(1, 2, 3)
    vp = ctypes.cast(arr, ctypes.c_void_p)
    args = (t, None, 7, 0.5, True, arr, vp)
    got = ops._marshal(args)
    assert len(got) == len(args)
    assert type(got[0]) is int and got[0] == t.data_ptr()
    for g, a in zip(got[1:], args[1:]):
        assert g is a
    view = t[2:]                                       # a view's pointer includes its storage offset
    assert ops._marshal([view]) == [t.data_ptr() + 8]
    assert ops._marshal(()) == []


def test_only_call_and_query_reach_the_library():
    for name, allowed in ALLOWED.items():
        users = _library_users(os.path.join(PKG, name))
        helpers = {"_call", "_query"} if name == "ops.py" else set()
        assert helpers <= users, f"{name}: {sorted(helpers - users)} no longer reach the library"
        extra = users - helpers - set(allowed)
        assert not extra, (f"{name}: {sorted(extra)} use _lib.lib / _lib.check directly: go through ops._call / ops._query, "
                           f"or add the function to ALLOWED with its reason")
        stale = set(allowed) - users
        assert not stale, f"{name}: ALLOWED lists {sorted(stale)}, which no longer reference the library"
        assert all(isinstance(why, str) and why for why in allowed.values())


def test_query_asks_the_built_library():
    build.build()
    assert ops._query("tpspp_bn_pool2x2_bwd_reduce_workspace_floats", 2, 3, 4, 4) == 6
    assert ops.bn_pool2x2_bwd_reduce_workspace_floats(2, 3, 4, 4) == 6
