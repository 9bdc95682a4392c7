"""Poison every device buffer an engine keeps between calls (tests/test_engine_reuse_gpu.py, tests/test_workspace_poison_cpu.py).

The engines of cbfssm.hip.ops / train / train_half allocate their workspaces with torch.zeros and keep them for life, and
every parity test starts from a fresh engine: a kernel that reads a lane, row block, slab or slot it never wrote gets exact
zeros there and passes.  `poison` overwrites the whole STORAGE of every floating-point tensor reachable from an engine (the
part of a tile pool beyond the current view and retired pools included) with a 32-bit word pattern; an engine that owns what
it reads gives the bits of a fresh engine afterwards.

Needs torch only: no GPU, no library (the walk recognises the project's classes by their module name).
"""
import ctypes
import fnmatch
import types

import numpy as np
import torch

# 32-bit patterns.  Both readings matter: the float32 kept records of a float32 engine live in a float64 tile pool.
#   nan   0x7ff80000 0x7ff80000 is a quiet NaN as float64, 0x7ff80000 a quiet NaN as float32, its high half 0x7ff8 one as bf16
#   huge  0x7e967699 0x7e967699 is about 5e301 as float64 and about 1e38 as float32: finite and enormous in both
# NaN alone is lost in fmax / compares, a finite value alone is lost in a product with an exact zero: both words run.
WORDS = {'nan': 0x7ff80000, 'huge': 0x7e967699}

# State that must survive between calls: (pattern, reason).  A pattern is `<class name>.<path below an instance of it>`,
# fnmatch syntax, matched against every object of that class on the way to a tensor.  A kept path wins for its whole storage.
# Nothing else belongs here: a buffer that must survive and is not optimiser state or pre-drawn noise is a finding.
KEEP = (
    ('TFAdam.flat', 'the parameters themselves (the views in TFAdam.views / HipTrainStep.params share this storage)'),
    ('TFAdam.m', 'first-moment estimate of the optimiser'),
    ('TFAdam.v', 'second-moment estimate of the optimiser'),
    ('TFAdam.t_dev', 'step counter of the optimiser as its update kernel reads it'),
    ('NoisePipeline._bufs*', 'pre-drawn noise of the next evaluation'),
)

PROJECT = 'cbfssm.hip'
_FLOAT = (torch.float64, torch.float32, torch.float16, torch.bfloat16)


def _project_instance(obj):
    mod = getattr(type(obj), '__module__', '') or ''
    return mod == PROJECT or mod.startswith(PROJECT + '.')


def _skip(obj):
    """never entered: modules, callables, ctypes data, numpy arrays (streams, events, graphs, generators and process groups
    are no plain containers and no project classes: they fall out by themselves)"""
    return (isinstance(obj, (types.ModuleType, np.ndarray, ctypes._SimpleCData, ctypes.Structure, ctypes.Union, ctypes.Array,
                             ctypes._Pointer, str, bytes)) or callable(obj))


class Group:
    """one storage: every path that reaches it"""

    def __init__(self, tensor):
        self.tensor = tensor                 # any tensor of the storage (keeps it alive, gives device and storage)
        self.paths, self.dtypes, self.kept_by = [], set(), []
        self.poisoned = False

    @property
    def nbytes(self):
        return int(self.tensor.untyped_storage().nbytes())


class Report:
    def __init__(self):
        self.groups = {}                     # (device, storage pointer) -> Group
        self.nonfloat = []                   # (path, dtype, bytes): listed, left alone

    def poisoned(self):
        return [g for g in self.groups.values() if g.poisoned]

    def kept(self):
        return [g for g in self.groups.values() if g.kept_by]

    def poisoned_paths(self):
        return [p for g in self.poisoned() for p in g.paths]

    def poisoned_bytes(self):
        return sum(g.nbytes for g in self.poisoned())

    def lines(self, max_paths=3):
        """one line per storage, the shortest paths first"""
        out = []
        for g in sorted(self.groups.values(), key=lambda g: min(g.paths, key=len)):
            what = 'kept (%s)' % ', '.join(g.kept_by) if g.kept_by else ('poisoned' if g.poisoned else 'found')
            paths = sorted(g.paths, key=len)
            more = ' (+%d more)' % (len(paths) - max_paths) if len(paths) > max_paths else ''
            out.append('%-9s %10d B  %s  %s' % (what.split(' ')[0], g.nbytes, '/'.join(sorted(str(d)[6:] for d in g.dtypes)),
                                               ', '.join(paths[:max_paths]) + more) + (('   <- ' + what) if g.kept_by else ''))
        out += ['non-float %10d B  %s  %s' % (n, str(d)[6:], p) for p, d, n in self.nonfloat]
        return out


def _kept_by(typed, keep):
    return [pat for pat, _ in keep for t in typed if fnmatch.fnmatchcase(t, pat)]


def reachable_storages(root, keep=KEEP, project=_project_instance):
    """Walk root's object graph -- instance __dict__s, dict values, list / tuple items; plain containers, SimpleNamespaces
    and instances of classes defined under cbfssm.hip only -- and group the floating-point tensors by storage."""
    rep = Report()
    # (object, path, typed: `<class>.<path below it>` for every project object on the way, ids of the objects on the way).
    # An object shared by two owners is walked once per owner, so that every path is reported; an object that is its own
    # ancestor is not entered again: that is what makes the walk cycle-safe.
    stack = [(root, type(root).__name__, [type(root).__name__] if project(root) else [], frozenset())]
    while stack:
        obj, path, typed, above = stack.pop()
        if isinstance(obj, torch.Tensor):
            if obj.dtype not in _FLOAT:
                rep.nonfloat.append((path, obj.dtype, obj.numel() * obj.element_size()))
                continue
            st = obj.untyped_storage()
            key = (str(obj.device), st.data_ptr())
            g = rep.groups.get(key)
            if g is None:
                g = rep.groups[key] = Group(obj)
            if path not in g.paths:
                g.paths.append(path)
            g.dtypes.add(obj.dtype)
            for pat in _kept_by(typed, keep):
                if pat not in g.kept_by:
                    g.kept_by.append(pat)
            continue
        if obj is None or isinstance(obj, (int, float, bool, complex)) or _skip(obj):
            continue
        if id(obj) in above:
            continue
        children = []
        if isinstance(obj, dict):
            children += [('[%r]' % (k,), v) for k, v in obj.items()]
        elif isinstance(obj, (list, tuple)):
            children += [('[%d]' % i, v) for i, v in enumerate(obj)]
        elif not (isinstance(obj, types.SimpleNamespace) or project(obj)):
            continue
        if hasattr(obj, '__dict__') and (isinstance(obj, types.SimpleNamespace) or project(obj)):
            children += [('.' + k, v) for k, v in vars(obj).items()]
        above = above | {id(obj)}
        for suffix, child in children:
            ctyped = [t + suffix for t in typed]
            if project(child) and not isinstance(child, torch.Tensor):
                ctyped.append(type(child).__name__)
            stack.append((child, path + suffix, ctyped, above))
    return rep


def _sync(rep):
    if any(g.tensor.is_cuda for g in rep.groups.values()) and torch.cuda.is_available():
        torch.cuda.synchronize()


def poison(root, word, keep=KEEP, project=_project_instance):
    """Overwrite the whole storage of every floating-point tensor reachable from root that KEEP does not name with the
    32-bit `word`; returns the Report (paths, dtypes, bytes; what was kept and by which pattern)."""
    rep = reachable_storages(root, keep, project)
    _sync(rep)
    word = int(word) & 0xffffffff
    signed = word - (1 << 32) if word >= 1 << 31 else word
    for g in rep.groups.values():
        if g.kept_by:
            continue
        st = g.tensor.untyped_storage()
        n = int(st.nbytes())
        if n >= 4:
            torch.empty(0, dtype=torch.int32, device=g.tensor.device).set_(st, 0, (n // 4,), (1,)).fill_(signed)
        if n % 4:                            # a trailing half word (16-bit dtypes): the pattern's next bytes
            tail = torch.empty(0, dtype=torch.uint8, device=g.tensor.device).set_(st, n - n % 4, (n % 4,), (1,))
            tail.copy_(torch.tensor([(word >> (8 * i)) & 0xff for i in range(n % 4)], dtype=torch.uint8))
        g.poisoned = n > 0
    _sync(rep)
    return rep
