"""Poison every per-call buffer of the GPModel surface (tests/test_gp_surface_poison_gpu.py,
tests/test_gp_surface_poison_cpu.py).

cbfssm.hip.autograd, cbfssm.hip.ops and cbfssm.model.gp_tf allocate what a call needs -- outputs, work buffers, the slabs of
the adjoints, the records a forward keeps for its backward -- with torch.empty / torch.empty_like.  In a test process those
come back as zero pages or as the finite values of the previous, often identical, call: a kernel that reads a padding row, a
lane of a ragged group, a scratch slab or an unconditioned step's record without having written it in this call passes.

    with poisoned_allocations(word) as log:
        ...

fills, for its duration, every tensor torch.empty / torch.empty_like return over its whole storage with the 32-bit `word`
(the int32-view fill of tests/workspace_poison.py: both readings of the word matter) and logs it: calling function, file,
line, the name it is assigned to, shape and bytes.  The patch is on the Python attributes of `torch`, so it sees exactly the
allocations made from Python -- the glue under test -- and is undone on exit, exceptions included.  Product code is not
changed for it.  The three product files use no other uninitialised allocator (source_allocations() scans for
ALLOCATOR_CALLS and the CPU test pins that nothing else of the kind -- new_empty, empty_strided, resize_ -- appears).

WORDS adds the baseline word 0 to workspace_poison.WORDS: a run on zero-filled allocations, which is what a fresh process
usually sees.  poison_pack(gp, word) poisons the model's own pack: every entry point re-prepares it, so nothing may read a
section `prepare` does not write.

Needs torch only: no GPU, no library."""
import ast
import collections
import contextlib
import os
import sys

import torch

import workspace_poison as wp

WORDS = dict(wp.WORDS, zero=0x00000000)
ORDER = ('zero', 'nan', 'huge')              # the baseline first
PATCHED = ('empty', 'empty_like')
# what a scan of the product files looks for: every way to get uninitialised memory from torch
ALLOCATOR_CALLS = ('empty', 'empty_like', 'empty_strided', 'new_empty', 'new_empty_strided', 'resize_', 'empty_permuted')

_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cbf-ssm_amd', 'cbfssm')
PRODUCT_FILES = {'autograd.py': os.path.join(_PKG, 'hip', 'autograd.py'), 'ops.py': os.path.join(_PKG, 'hip', 'ops.py'),
                 'gp_tf.py': os.path.join(_PKG, 'model', 'gp_tf.py')}

Alloc = collections.namedtuple('Alloc', 'func file line name shape nbytes')


class Log(list):
    """the allocations of one context, in order"""

    def sites(self):
        """{(file, line)} that allocated at least one byte or were reached at all"""
        return {(a.file, a.line) for a in self}

    def by_function(self):
        out = collections.OrderedDict()
        for a in self:
            out.setdefault((a.file, a.func), []).append(a)
        return out

    def product(self):
        """the entries whose call site is in one of the three product files"""
        return Log(a for a in self if a.file in PRODUCT_FILES)

    def nbytes(self):
        return sum(a.nbytes for a in self)


def _fill(t, word):
    """the whole storage of t, through workspace_poison.poison (floating point) or the same int32 view (anything else)"""
    if t.untyped_storage().nbytes() == 0:
        return
    if t.dtype in wp._FLOAT:
        wp.poison(t, word, keep=())
        return
    word = int(word) & 0xffffffff
    signed = word - (1 << 32) if word >= 1 << 31 else word
    st = t.untyped_storage()
    n = int(st.nbytes())
    if n >= 4:
        _ORIG['empty'](0, dtype=torch.int32, device=t.device).set_(st, 0, (n // 4,), (1,)).fill_(signed)
    if n % 4:
        tail = _ORIG['empty'](0, dtype=torch.uint8, device=t.device).set_(st, n - n % 4, (n % 4,), (1,))
        tail.copy_(torch.tensor([(word >> (8 * i)) & 0xff for i in range(n % 4)], dtype=torch.uint8))


_ORIG = {name: getattr(torch, name) for name in PATCHED}
_STATE = {'busy': False}


def _call_site(frame):
    """(function, file base name or path, line) of the frame that called the allocator; a lambda is named after the
    function that called it (the `new = lambda ...` idiom of the glue defines and calls it in one function)"""
    code = frame.f_code
    func = code.co_name
    if func == '<lambda>' and frame.f_back is not None:
        func = frame.f_back.f_code.co_name + '.<lambda>'
    path = code.co_filename
    base = os.path.basename(path)
    known = PRODUCT_FILES.get(base)
    file = base if known is not None and os.path.abspath(path) == os.path.abspath(known) else path
    return func, file, frame.f_lineno


@contextlib.contextmanager
def poisoned_allocations(word):
    log = Log()
    state = _STATE                           # (module-wide: a nested context's fill is not poisoned by the outer one)
    saved = {name: getattr(torch, name) for name in PATCHED}
    names = _assigned_names()

    def patched(name):
        orig = saved[name]

        def alloc(*args, **kwargs):
            t = orig(*args, **kwargs)
            if state['busy'] or not isinstance(t, torch.Tensor):
                return t
            state['busy'] = True             # (the fill itself allocates its int32 view with torch.empty)
            try:
                _fill(t, word)
                func, file, line = _call_site(sys._getframe(1))
                log.append(Alloc(func, file, line, names.get((file, line)), tuple(t.shape),
                                 int(t.untyped_storage().nbytes())))
            finally:
                state['busy'] = False
            return t
        alloc.__name__ = name
        return alloc

    try:
        for name in PATCHED:
            setattr(torch, name, patched(name))
        yield log
    finally:
        for name in PATCHED:
            setattr(torch, name, saved[name])


def poison_pack(gp, word):
    """workspace_poison.poison on the model's own pack (re-prepared by every entry point)"""
    return wp.poison(gp._pack, word)


# ---- the allocation sites of the product files, from the source text
Site = collections.namedtuple('Site', 'file func line name call')


def _target_names(node):
    if isinstance(node, ast.Name):
        return [node.id]
    if isinstance(node, (ast.Tuple, ast.List)):
        return [n for e in node.elts for n in _target_names(e)]
    if isinstance(node, ast.Attribute):
        return [node.attr]
    return []


def _alloc_calls(node):
    return [c for c in ast.walk(node) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)
            and c.func.attr in ALLOCATOR_CALLS]


_SITES = None


def source_allocations():
    """every call of an uninitialised allocator in the three product files: [Site(file, func, line, name, call)], `func` the
    enclosing function (Class.method for methods), `name` what the result is assigned to (a tuple assignment with several
    allocations gives one site per allocation, in order), `call` the allocator's attribute name"""
    global _SITES
    if _SITES is not None:
        return _SITES
    out = []
    for base, path in PRODUCT_FILES.items():
        with open(path) as f:
            tree = ast.parse(f.read(), path)

        def visit(node, qual):
            for child in ast.iter_child_nodes(node):
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    visit(child, qual + [child.name])
                elif isinstance(child, ast.ClassDef):
                    visit(child, qual + [child.name])
                elif isinstance(child, ast.stmt):
                    calls = _alloc_calls(child) if not _has_nested_stmts(child) else []
                    if calls:
                        names = _target_names(child.targets[0]) if isinstance(child, ast.Assign) else []
                        calls.sort(key=lambda c: (c.lineno, c.col_offset))
                        for i, c in enumerate(calls):
                            nm = names[i] if len(names) == len(calls) else (names[0] if len(names) == 1 else None)
                            out.append(Site(base, '.'.join(qual) or '<module>', c.lineno, nm, c.func.attr))
                    visit(child, qual)
        visit(tree, [])
    _SITES = sorted(set(out), key=lambda s: (s.file, s.line, s.name or ''))
    return _SITES


def _has_nested_stmts(node):
    return any(isinstance(c, ast.stmt) for c in ast.iter_child_nodes(node))


def _assigned_names():
    names = {}
    for s in source_allocations():
        key = (s.file, s.line)
        names[key] = s.name if key not in names else '%s, %s' % (names[key], s.name)
    return names


def sites_of(*funcs):
    """the sites of the named functions ('file:func'), e.g. sites_of('autograd.py:_gp_tail')"""
    want = set(funcs)
    got = [s for s in source_allocations() if '%s:%s' % (s.file, s.func) in want]
    missing = want - {'%s:%s' % (s.file, s.func) for s in got}
    assert not missing, 'no allocation site in %s' % sorted(missing)
    return got
