"""tests/workspace_poison.py on a synthetic object graph of CPU tensors: what the walk finds, what it leaves alone, that a
storage is overwritten once and whole, and what the two words read as."""
import types

import numpy as np
import torch

import workspace_poison as wp


def _cls(name, module='cbfssm.hip.synthetic_graph'):
    return type(name, (), {'__module__': module})


Engine, TFAdam, NoisePipeline, Pool = _cls('Engine'), _cls('TFAdam'), _cls('NoisePipeline'), _cls('Pool')
Foreign = _cls('Foreign', 'somewhere.else')


def _graph():
    e = Engine()
    e.red = torch.zeros(7, dtype=torch.float64)
    e.pool = Pool()
    base = torch.arange(64, dtype=torch.float64)
    e.pool.bufs = (base[8:24], None)                                  # a view into a larger buffer ...
    e.pool.retired = [[torch.ones(5, dtype=torch.float32)]]
    e._ws = {(2, 7): types.SimpleNamespace(a2s=base[8:16].view(2, 4), x=torch.zeros(3, 2), idx=torch.arange(4)),
             ('eval', 2, 7): {'half': torch.zeros(3, dtype=torch.bfloat16), 'odd': torch.zeros(3, dtype=torch.float16)}}
    e.last_ws = e._ws[(2, 7)]                                          # a second path to the same object
    e.opt = TFAdam()
    e.opt.flat = torch.full((6,), 3.0, dtype=torch.float64)
    e.opt.views = {'a': e.opt.flat[:2], 'b': e.opt.flat[2:]}          # not named in KEEP: kept through the storage
    e.opt.m, e.opt.v, e.opt.t_dev = torch.full((6,), 4.0), torch.full((6,), 5.0), torch.full((1,), 6.0)
    e.opt.gflat = torch.zeros(6, dtype=torch.float64)                 # scratch of the optimiser: not kept
    e.params = e.opt.views
    e.noise = NoisePipeline()
    e.noise._bufs = {(5, 8): [torch.full((4,), 7.0), torch.full((4,), 8.0)]}
    e.self = e                                                         # cycles
    e._ws['back'] = [e, e._ws]
    e.foreign = Foreign()
    e.foreign.t = torch.full((3,), 9.0)                                # an object of another package: not entered
    e.module, e.fn, e.array = types, (lambda: e.red), np.zeros(3)
    e.text, e.count = 'x', 3
    return e, base


def test_walk_finds_nested_tensors_and_every_path():
    e, base = _graph()
    rep = wp.reachable_storages(e)
    paths = {p for g in rep.groups.values() for p in g.paths}
    for want in ('Engine.red', 'Engine.pool.bufs[0]', 'Engine.pool.retired[0][0]', 'Engine._ws[(2, 7)].a2s',
                 'Engine._ws[(2, 7)].x', 'Engine.last_ws.x', "Engine._ws[('eval', 2, 7)]['half']", 'Engine.opt.flat',
                 "Engine.opt.views['a']", "Engine.params['b']", 'Engine.opt.gflat', 'Engine.noise._bufs[(5, 8)][1]'):
        assert want in paths, (want, sorted(paths))
    assert not any('foreign' in p or 'array' in p or 'fn' in p for p in paths)
    assert sorted((p, d) for p, d, _ in rep.nonfloat) == [('Engine._ws[(2, 7)].idx', torch.int64),
                                                           ('Engine.last_ws.idx', torch.int64)]
    # two views of one storage are one group with both paths
    g = rep.groups[(str(base.device), base.untyped_storage().data_ptr())]
    assert {'Engine.pool.bufs[0]', 'Engine._ws[(2, 7)].a2s', 'Engine.last_ws.a2s'} <= set(g.paths) and g.nbytes == 64 * 8


def test_poison_writes_the_whole_storage_once_and_keeps_state():
    for word in wp.WORDS.values():
        e, base = _graph()
        rep = wp.poison(e, word)
        raw = np.frombuffer(base.numpy().tobytes(), dtype=np.uint32)
        assert raw.size == 128 and (raw == word).all()                 # elements outside both views included
        for t in (e.red, e.pool.retired[0][0], e.last_ws.x, e.opt.gflat, e._ws[('eval', 2, 7)]['half']):
            n = t.untyped_storage().nbytes()
            b = np.frombuffer(bytes(t.untyped_storage().tolist()), dtype=np.uint8)
            assert (b[:n - n % 4].view(np.uint32) == word).all(), t.dtype
        odd = bytes(e._ws[('eval', 2, 7)]['odd'].untyped_storage().tolist())      # six bytes: a word and a half
        assert odd == (word.to_bytes(4, 'little') * 2)[:6]
        # kept: the optimiser's state (the views through their storage) and the pre-drawn noise; the report says why
        assert torch.equal(e.opt.flat, torch.full((6,), 3.0, dtype=torch.float64))
        assert float(e.opt.m[0]) == 4.0 and float(e.opt.v[0]) == 5.0 and float(e.opt.t_dev) == 6.0
        assert [float(b[0]) for b in e.noise._bufs[(5, 8)]] == [7.0, 8.0]
        kept = {p: g.kept_by for g in rep.kept() for p in g.paths}
        assert kept["Engine.params['a']"] == ['TFAdam.flat'] and kept['Engine.noise._bufs[(5, 8)][0]'] == ['NoisePipeline._bufs*']
        assert not any(g.poisoned for g in rep.kept())
        # left alone: integers, objects of other packages
        assert torch.equal(e.last_ws.idx, torch.arange(4)) and float(e.foreign.t[0]) == 9.0
        assert 'Engine.red' in rep.poisoned_paths() and rep.poisoned_bytes() >= 64 * 8
        assert any('kept' in line and 'TFAdam.flat' in line for line in rep.lines())


def test_keep_can_be_replaced_and_a_kept_view_wins_for_its_storage():
    e, base = _graph()
    rep = wp.poison(e, wp.WORDS['nan'], keep=(('Pool.bufs*', 'test'),))
    assert torch.equal(base, torch.arange(64, dtype=torch.float64))    # the whole storage, although only a view is named
    assert torch.isnan(e.opt.flat).all() and torch.isnan(e.noise._bufs[(5, 8)][0]).all()
    g = rep.groups[(str(base.device), base.untyped_storage().data_ptr())]
    assert g.kept_by == ['Pool.bufs*'] and 'Engine.last_ws.a2s' in g.paths


def test_words_read_as_stated():
    for name, word in wp.WORDS.items():
        t = torch.zeros(4, dtype=torch.float64)
        holder = types.SimpleNamespace(t=t)
        wp.poison(holder, word)
        f64, f32, b16 = t, t.view(torch.float32), t.view(torch.bfloat16)
        if name == 'nan':
            assert torch.isnan(f64).all() and torch.isnan(f32).all()
            assert torch.isnan(b16[1::2]).all()                        # the high half of every word (little endian)
        else:
            assert torch.isfinite(f64).all() and torch.isfinite(f32).all()
            assert float(f64.abs().min()) > 1e30 and float(f32.abs().min()) > 1e30
