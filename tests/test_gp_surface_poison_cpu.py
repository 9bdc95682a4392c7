"""tests/gp_surface_poison.py without a GPU: the context manager poisons and logs what torch.empty / torch.empty_like hand
out, takes its patch back whatever happens, and the source scan finds every uninitialised allocation of the three product
files -- all of them torch.empty or torch.empty_like, which is what the patch covers."""
import numpy as np
import pytest
import torch

import gp_surface_poison as gsp
import workspace_poison as wp


def _words(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


def test_words_come_from_workspace_poison_plus_the_baseline():
    assert gsp.WORDS['nan'] is wp.WORDS['nan'] and gsp.WORDS['huge'] is wp.WORDS['huge']
    assert gsp.WORDS['zero'] == 0 and set(gsp.WORDS) == set(wp.WORDS) | {'zero'}
    assert gsp.ORDER[0] == 'zero' and set(gsp.ORDER) == set(gsp.WORDS)


@pytest.mark.parametrize('name', gsp.ORDER)
def test_a_tensor_allocated_inside_the_context_carries_the_word(name):
    word = gsp.WORDS[name]
    with gsp.poisoned_allocations(word) as log:
        a = torch.empty(5, 3, dtype=torch.float64)
        b = torch.empty_like(a)
        c = torch.empty(7, dtype=torch.float32)
        d = torch.empty(3, dtype=torch.int64)
        e = torch.empty(0, dtype=torch.float64)
        h = torch.empty(3, dtype=torch.float16)                  # six bytes: a trailing half word
    for t in (a, b, c, d):
        assert np.all(_words(t) == word), name
    assert np.all(h.view(torch.int16).numpy().view(np.uint16) == [word & 0xffff, word >> 16, word & 0xffff])
    if name == 'nan':
        assert torch.isnan(a).all() and torch.isnan(b).all() and torch.isnan(c).all()
    if name == 'huge':
        assert torch.isfinite(a).all() and float(a.min()) > 1e300 and float(c.min()) > 1e37
    assert [x.shape for x in log] == [(5, 3), (5, 3), (7,), (3,), (0,), (3,)]
    assert [x.nbytes for x in log] == [120, 120, 28, 24, 0, 6] and log.nbytes() == 298
    assert e.numel() == 0


def test_the_log_names_the_call_site():
    def some_glue():
        return torch.empty(4, dtype=torch.float64)
    new = lambda *s: torch.empty(*s, dtype=torch.float64)      # noqa: E731  (the idiom of cbfssm.hip.autograd)

    def with_lambda():
        return new(2, 2)
    with gsp.poisoned_allocations(gsp.WORDS['nan']) as log:
        some_glue()
        line = some_glue.__code__.co_firstlineno + 1
        with_lambda()
    assert len(log) == 2
    assert log[0].func == 'some_glue' and log[0].file == __file__ and log[0].line == line
    assert log[0].shape == (4,) and log[0].nbytes == 32
    assert log[1].func == 'with_lambda.<lambda>' and log[1].file == __file__
    assert log.sites() == {(__file__, line), (__file__, new.__code__.co_firstlineno)}
    assert list(log.by_function()) == [(__file__, 'some_glue'), (__file__, 'with_lambda.<lambda>')]
    assert log.product() == []


def test_the_patch_is_gone_after_the_context_and_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    with gsp.poisoned_allocations(gsp.WORDS['nan']):
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(ZeroDivisionError):
        with gsp.poisoned_allocations(gsp.WORDS['huge']):
            torch.empty(3)
            1 / 0
    assert torch.empty is empty and torch.empty_like is empty_like
    # an allocator that raises leaves the context usable and the patch removable
    with gsp.poisoned_allocations(gsp.WORDS['nan']) as log:
        with pytest.raises(TypeError):
            torch.empty('three')
        t = torch.empty(2, dtype=torch.float64)
    assert torch.isnan(t).all() and len(log) == 1 and torch.empty is empty
    # outside, nothing is filled or logged
    assert not torch.isnan(torch.zeros(2) + torch.empty(2).fill_(1.0)).any()


def test_nested_contexts_restore_in_order():
    empty = torch.empty
    with gsp.poisoned_allocations(gsp.WORDS['nan']) as outer:
        with gsp.poisoned_allocations(gsp.WORDS['huge']) as inner:
            torch.empty(1, dtype=torch.float64)
        t = torch.empty(1, dtype=torch.float64)
    assert torch.empty is empty and len(inner) == 1 and torch.isnan(t).all() and len(outer) >= 1


def test_poison_of_a_pack_like_object_goes_through_workspace_poison():
    class Pack:                                                   # (a project class as the walk recognises it)
        pass
    Pack.__module__ = 'cbfssm.hip.ops'
    gp = type('GP', (), {})()
    gp._pack = Pack()
    gp._pack.buf = torch.zeros(9, dtype=torch.float64)
    rep = gsp.poison_pack(gp, gsp.WORDS['nan'])
    assert torch.isnan(gp._pack.buf).all() and rep.poisoned_bytes() == 72


def test_the_source_scan_finds_the_allocations_of_the_three_product_files():
    sites = gsp.source_allocations()
    assert {s.file for s in sites} == set(gsp.PRODUCT_FILES)
    # nothing but torch.empty / torch.empty_like: what the context manager patches is all there is
    assert {s.call for s in sites} == set(gsp.PATCHED)
    # the scan agrees with a plain text search, line by line
    for base, path in gsp.PRODUCT_FILES.items():
        with open(path) as f:
            lines = [i + 1 for i, l in enumerate(f) if 'torch.empty' in l.split('#')[0]]
        assert sorted({s.line for s in sites if s.file == base}) == lines, base
        with open(path) as f:
            text = f.read()
        for other in set(gsp.ALLOCATOR_CALLS) - set(gsp.PATCHED):
            assert '.%s(' % other not in text, (base, other)
    by = {(s.file, s.func, s.name) for s in sites}
    for key in (('autograd.py', '_GpPredict.backward', 'gpart'), ('autograd.py', '_GpPredict.backward', 'image'),
                ('autograd.py', '_gp_tail', 'work'), ('autograd.py', 'gp_eks_eval', 'new'),
                ('autograd.py', '_GpEkf.backward', 'gm0'), ('autograd.py', '_GpEkf.backward', 'gy'),
                ('ops.py', 'GPPack.predict', 'fvar'), ('gp_tf.py', 'cast_cholesky', 'work'), ('gp_tf.py', 'RBF.K', 'out')):
        assert key in by, key
    assert len(sites) >= 90
    assert len(gsp.sites_of('autograd.py:_gp_tail')) == 2
    with pytest.raises(AssertionError):
        gsp.sites_of('autograd.py:no_such_function')


def test_every_allocation_site_belongs_to_a_table_of_the_gpu_file():
    """the static half of the coverage guard: a new torch.empty in one of the three product files is in a function that some
    entry point's table names -- then the guard of tests/test_gp_surface_poison_gpu.py demands that it was poisoned -- or
    this fails until a case reaches it (EXEMPT holds what is deliberately left to another file, with the reason)"""
    import test_gp_surface_poison_gpu as tgpu
    named = {f for funcs in tgpu.TABLES.values() for f in funcs}
    have = {'%s:%s' % (s.file, s.func) for s in gsp.source_allocations()}
    assert not named & set(tgpu.EXEMPT)
    assert have - named == set(tgpu.EXEMPT), sorted(have - named - set(tgpu.EXEMPT))
    assert named <= have, sorted(named - have)
    # every table is used by a test of the file, and every conditional name the guard knows exists in the source
    text = open(tgpu.__file__).read()
    for entry in tgpu.TABLES:
        assert "'%s'" % entry in text.split('TABLES = {')[1].split('\n}\n', 1)[1], entry
    names = {s.name for s in gsp.source_allocations()}
    assert {'image', 'work', 'vsave', 'msave', 'ga', 'dvar', 'xcov', 'gP0', 'new'} <= names
    funcs = {s.func for s in gsp.source_allocations()}
    assert tgpu.STASH_WORK <= funcs and set(tgpu.LAMBDA_COUNTS) <= funcs


def test_the_guard_fails_when_an_allocation_is_not_poisoned_or_not_expected():
    """the guard itself, on synthetic logs: complete passes; one line missing, one stray line and a wrong mode each fail"""
    import test_gp_surface_poison_gpu as tgpu
    flags = dict(stash=False, grad=False, has_a=True, variance=True, cross=True, lag_one=False, has_P0=True)
    sites = gsp.sites_of(*tgpu.TABLES['linearize'])

    def log_of(ss):
        return gsp.Log(gsp.Alloc(s.func, s.file, s.line, s.name, (3,), 24) for s in ss)
    tgpu._guard('linearize', log_of(sites), flags)
    with pytest.raises(AssertionError, match='not poisoned'):
        tgpu._guard('linearize', log_of(sites[1:]), flags)
    with pytest.raises(AssertionError, match='should not'):
        tgpu._guard('linearize', log_of(sites), dict(flags, variance=False))
    stray = gsp.sites_of('autograd.py:_gp_tail')[:1]
    with pytest.raises(AssertionError, match='outside the table'):
        tgpu._guard('linearize', log_of(sites + stray), flags)
    # a stash-only buffer is demanded at the stash heights and refused below them
    sites = gsp.sites_of(*tgpu.TABLES['predict_grad'])
    low = [s for s in sites if s.name not in ('image', 'work') or s.func == '_gp_tail']
    tgpu._guard('predict_grad', log_of(low), dict(flags, grad=True))
    with pytest.raises(AssertionError, match='not poisoned'):
        tgpu._guard('predict_grad', log_of(low), dict(flags, grad=True, stash=True))
    tgpu._guard('predict_grad', log_of(sites), dict(flags, grad=True, stash=True))
