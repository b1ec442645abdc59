"""The door of the C-ABI, checked in the source: every exported function that takes a context passes nif_enter / NIF_ENTER (nif_ctx.h) in
its own body, where it names the deferred state it runs (NIF_FLUSH_NONE, _TAIL or _METRIC).  No library build, no GPU."""
import ctypes as C
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The exports that pass no guard.  The condition for being listed: the function touches NO device state of the context at all -- it
# selects no device, enqueues nothing, reads or writes no device buffer -- so there is nothing a deferred piece could be stale for.
# Everything else is guarded, with NIF_FLUSH_NONE as the explicit class where the entry point runs neither deferred piece.  Delegating
# to a guarded function is not a reason.
UNGUARDED = {
    "nif_param_count": "accessor: a size fixed at nif_create",
    "nif_po_dim": "accessor: a size fixed at nif_create",
    "nif_param_layout": "accessor: the host copy of the layout, fixed at nif_create",
    "nif_stream": "accessor: returns the stream handle",
    "nif_params_dev": "accessor: returns the address of theta, reads nothing",
    "nif_comm_info": "accessor: rank and world size, host fields",
    "nif_set_option": "sets host fields (fp32_mfma also marks the planes stale, a host flag); read by the next step",
    "nif_set_regularizer": "sets host fields; apply_reg reads them at the next consumer of the gradient",
    "nif_set_shapenet_regularizer": "sets host fields; apply_reg reads them at the next consumer of the gradient",
    "nif_set_jac_regularizer": "sets a host field, judged on the host; read by the next step",
    "nif_set_loss": "sets a host field; read by the next step",
    "nif_set_activity_regularizer": "sets host fields; read by the next step",
}

_GUARD = re.compile(r"\b(?:NIF_ENTER|nif_enter)\s*\(\s*[^,()]+(?:\[[^\]]*\])?\s*,\s*NIF_FLUSH_(?:NONE|TAIL|METRIC)\s*\)")
_DEF = re.compile(r'extern\s+"C"\s+[\w\s\*]+?\b(nif_\w+)\s*\(([^)]*)\)\s*\{')


def _code(txt):
    """the source without comments and string literals (a brace or a guard inside either does not count)"""
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r'"(?:\\.|[^"\\\n])*"', lambda m: '"C"' if m.group(0) == '"C"' else '""', txt)
    return re.sub(r"//[^\n]*", " ", txt)


def _exports():
    """name -> (first parameter, body) of every extern "C" definition in nif_amd/csrc/*.hip"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "nif_amd", "csrc", "*.hip"))):
        txt = _code(open(path).read())
        for m in _DEF.finditer(txt):
            depth, i = 1, m.end()
            while depth:
                depth += {"{": 1, "}": -1}.get(txt[i], 0)
                i += 1
            assert m.group(1) not in out, "%s is defined twice" % m.group(1)
            out[m.group(1)] = (" ".join(m.group(2).split(",")[0].split()), txt[m.end():i])
    return out


def _takes_ctx(first_param):
    return re.match(r"^nif_ctx\s*\*{1,2}\s*\w+$", first_param) is not None


def test_every_context_entry_point_passes_the_guard():
    from nif_amd import _lib
    exports = _exports()
    found = {n: body for n, (first, body) in exports.items() if _takes_ctx(first)}
    # the parser sees every export and not a subset: the context-taking functions of the ctypes tables, which mirror the headers one to
    # one (tests/test_abi.py).  ctypes spells nif_ctx* and void* alike: nif_comm_unique_id's only parameter is `void* id_out`
    table = dict(_lib.SIGNATURES, **_lib.SNAPSHOT_SIGNATURES)
    ctx_types = (_lib._CTX, C.POINTER(_lib._CTX))
    want = {n for n, (_, args) in table.items() if args and args[0] in ctx_types} - {"nif_comm_unique_id"}
    assert set(found) == want, "parser and ctypes tables disagree: %r" % sorted(set(found) ^ want)
    assert set(exports) >= set(table), "not found as extern \"C\" definitions: %r" % sorted(set(table) - set(exports))
    for name, reason in UNGUARDED.items():
        assert name in found, "UNGUARDED lists %s, which is no context-taking export" % name
        assert isinstance(reason, str) and reason.strip(), "UNGUARDED[%s] has no reason" % name
    missing = sorted(n for n, body in found.items() if n not in UNGUARDED and not _GUARD.search(body))
    assert not missing, "context-taking exports without nif_enter / NIF_ENTER in their own body: %r" % missing
    both = sorted(n for n in UNGUARDED if _GUARD.search(found[n]))
    assert not both, "listed as UNGUARDED but guarded: %r" % both
