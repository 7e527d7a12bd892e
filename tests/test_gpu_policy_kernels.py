"""The behavioural-cloning policy's kernels one by one - through the pvr_op_policy_* entry points, pvr_op_gemm_f32_masked and pvr_joint_apply_rmsprop,
which launch them with the plan's own launch code - against the float64 references and derived elementwise bounds of oracle/policy_kernel_refs.py.
Every output sits between guard rows holding a sentinel and is NaN before the launch; every input is a device allocation of its own, of exactly its
size; every test asserts error / bound <= 1 per family (the exact and impulse families and the integer outputs bit for bit), finiteness, untouched
guards and identical bits on a second run, and prints its worst ratios.  Two whole-step tests close the file: every gradient tensor, and the eval-mode
forward, at row counts on both sides of the 512-row dispatch boundary against float64 autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
from oracle import policy_kernel_refs as kr
from pvr_habitat_amd import _lib
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SENTINEL32 = 0x5A5A5A5A
NAN32 = 0x7FC00000
POISON64 = -0x5A5A5A5A5A5A5A5B                        # int64 outputs have no NaN: a value no kernel produces
GUARD = 4                                             # rows in front of and behind every output (four: a row of any width starts 16-byte aligned)
ROWS = (2, 7, 8, 9, 63, 64, 65, 130)
BOUNDARY = (511, 512, 513)
FORMS = [(r, f) for r in ROWS for f in (0, 1)] + [(r, -1) for r in BOUNDARY]
f32 = np.float32


def L():
    return M._plib()


def st():
    return _lib.stream_ptr()


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(t):
    """a device allocation of its own, of exactly the tensor's size"""
    return t.contiguous().cuda() if t is not None else None


class Out:
    """An output (or in/out buffer) of rows x cols between GUARD rows of a sentinel; NaN (a poison value for int64) before the launch unless `init`
    gives the in/out contents.  read() synchronises, checks the guards and returns the rows on the host."""

    def __init__(self, rows, cols, what, init=None, dtype=torch.float32):
        self.rows, self.cols, self.what, self.dtype = rows, cols, what, dtype
        self.it, self.sent = (torch.int32, SENTINEL32) if dtype == torch.float32 else (torch.int64, SENTINEL32)
        self.buf = torch.full((GUARD + rows + GUARD, cols), self.sent, dtype=self.it, device='cuda')
        if init is not None:
            self.buf[GUARD:GUARD + rows] = init.contiguous().view(rows, cols).view(self.it).cuda()
        else:
            self.buf[GUARD:GUARD + rows] = NAN32 if dtype == torch.float32 else POISON64

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.cols * self.buf.element_size())

    def read(self):
        torch.cuda.synchronize()
        o = self.buf.cpu()
        assert (o[:GUARD] == self.sent).all() and (o[GUARD + self.rows:] == self.sent).all(), '%s wrote outside its rows' % self.what
        return o[GUARD:GUARD + self.rows].view(self.dtype)


def twice(run, what):
    """run() -> dict of host tensors; two runs must agree in every bit"""
    a, b = run(), run()
    for k in a:
        assert kr.bits_equal(a[k], b[k]), '%s: two runs differ in %s' % (what, k)
    return a


def chk(got, refb, what, exact=False):
    ref, bound = refb
    assert torch.isfinite(got.float()).all(), '%s: a NaN survived or an output is not finite' % what
    got = got.reshape(ref.shape)
    if exact:
        assert torch.equal(got.double(), ref), '%s: not bit for bit' % what
    return kr.ratio(got, ref, bound)


def worst_of(d, k, r):
    d[k] = max(d.get(k, 0.0), r)


def report(tag, worst):
    print('\n[%s] error / bound %s' % (tag, {k: '%.2f' % v for k, v in sorted(worst.items())}))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def expect_form(form, R_, vec4, before, launches=1):
    """with form -1 the plan's choice must have been taken: the two-stage counter moved by `launches` per two-stage reduction, or not at all"""
    want = (kr.chosen_form(R_, vec4) if form < 0 else form) * launches
    assert L().pvr_debug_policy_two_stage_launches() - before == want, 'form %d at %d rows: the two-stage counter moved by %d, expected %d' % (
        form, R_, L().pvr_debug_policy_two_stage_launches() - before, want)
    return kr.chosen_form(R_, vec4) if form < 0 else form


# ------------------------------------------------------------------------------------------------------------------
# column reductions
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', FORMS, ids=lambda c: 'R%d_form%d' % c)
def test_colsum_matches_float64(case):
    R_, form = case
    worst = {}
    for Cc in (4, 36, 128, 132) + ((33,) if form != 1 else ()):
        for family in kr.REDUCE_FAMILIES:
            X = kr.reduce_inputs(family, R_, Cc)
            Xd = dev(X)
            second = Cc in (36, 132)                                            # the optional second output on some widths

            def run():
                o0, o1 = Out(1, Cc, 'colsum out0'), Out(1, Cc, 'colsum out1') if second else None
                before = L().pvr_debug_policy_two_stage_launches()
                _lib.check(L().pvr_op_policy_colsum(vp(Xd), o0.ptr, o1.ptr if second else None, R_, Cc, form, st()))
                run.form = expect_form(form, R_, Cc % 4 == 0, before)
                return dict(out0=o0.read(), **(dict(out1=o1.read()) if second else {}))
            got = twice(run, 'colsum R %d C %d %s' % (R_, Cc, family))
            refb = kr.colsum_ref(X, run.form)
            worst_of(worst, family, chk(got['out0'], refb, 'colsum R %d C %d %s' % (R_, Cc, family), exact=family != 'unit'))
            if second:
                assert kr.bits_equal(got['out0'], got['out1'])
    if form == 1:                                                               # a column count the float4 loads cannot take is refused, nothing is written
        o0 = Out(1, 33, 'refused colsum')
        assert L().pvr_op_policy_colsum(vp(dev(kr.reduce_inputs('unit', R_, 33))), o0.ptr, None, R_, 33, 1, st()) == 1 and 'multiple of 4' in _lib.last_error()
        assert torch.isnan(o0.read()).all()
    report('colsum R %d form %d' % case, worst)


def _rstats(Cc):
    return 0.5 * kr.rnd('bns.rm.%d' % Cc, (Cc,)), 0.5 + kr.rnd('bns.rv.%d' % Cc, (Cc,)).abs()


@pytest.mark.parametrize('case', FORMS, ids=lambda c: 'R%d_form%d' % c)
def test_bn_stats_matches_float64(case):
    R_, form = case
    worst = {}
    for Cc in (4, 36, 128, 132) + ((33,) if form == 0 else ()):
        X = kr.bn_inputs(R_, Cc, 'bns')['x']
        Xd = dev(X)
        rm, rv = _rstats(Cc)
        for mult in (1, 2):
            n = float(mult * R_)

            def run():
                o = {k: Out(1, Cc, 'bn_stats ' + k) for k in ('mean', 'invstd', 'sumsq')}
                o['running_mean'], o['running_var'] = Out(1, Cc, 'running_mean', init=rm), Out(1, Cc, 'running_var', init=rv)
                nbt = Out(1, 1, 'num_batches_tracked', init=torch.tensor([41], dtype=torch.int64), dtype=torch.int64)
                before = L().pvr_debug_policy_two_stage_launches()
                _lib.check(L().pvr_op_policy_bn_stats(vp(Xd), R_, Cc, n, form, o['mean'].ptr, o['invstd'].ptr, o['sumsq'].ptr, o['running_mean'].ptr,
                                                      o['running_var'].ptr, nbt.ptr, st()))
                run.form = expect_form(form, R_, Cc % 4 == 0, before, launches=2)
                res = {k: v.read() for k, v in o.items()}
                res['nbt'] = nbt.read()
                return res
            got = twice(run, 'bn_stats R %d C %d' % (R_, Cc))
            assert int(got['nbt']) == 42, 'num_batches_tracked must move by exactly one'
            for k, refb in kr.bn_stats_ref(X, n, rm, rv, run.form).items():
                worst_of(worst, '%s/n=%dR' % (k, mult), chk(got[k], refb, 'bn_stats %s R %d C %d' % (k, R_, Cc)))
    report('bn_stats R %d form %d' % case, worst)


@pytest.mark.parametrize('case', FORMS, ids=lambda c: 'R%d_form%d' % c)
def test_bn_backward_sums_match_float64(case):
    R_, form = case
    worst = {}
    for Cc in (4, 36, 128, 132) + ((33,) if form == 0 else ()):
        d = kr.bn_inputs(R_, Cc)
        for family in ('unit', 'impulse'):
            x, dy = d['x'], d['dy']
            if family == 'impulse':                                             # dy has one 1.0 per column (row 0 or the last row): dbeta is 1 bit for bit
                dy = (kr.reduce_inputs('impulse', R_, Cc) != 0).float()
            xd, dyd, md, sd = dev(x), dev(dy), dev(d['mean']), dev(d['invstd'])

            def run():
                o0, o1 = Out(1, Cc, 'dgamma'), Out(1, Cc, 'dbeta')
                before = L().pvr_debug_policy_two_stage_launches()
                _lib.check(L().pvr_op_policy_bn_backward_sums(vp(xd), vp(dyd), vp(md), vp(sd), o0.ptr, o1.ptr, R_, Cc, form, st()))
                run.form = expect_form(form, R_, Cc % 4 == 0, before)
                return dict(dgamma=o0.read(), dbeta=o1.read())
            got = twice(run, 'bn_backward_sums R %d C %d' % (R_, Cc))
            r0, r1 = kr.bn_backward_sums_ref(x, dy, d['mean'], d['invstd'], run.form)
            worst_of(worst, family + '/dgamma', chk(got['dgamma'], r0, 'dgamma R %d C %d' % (R_, Cc)))
            worst_of(worst, family + '/dbeta', chk(got['dbeta'], r1, 'dbeta R %d C %d' % (R_, Cc), exact=family == 'impulse'))
    report('bn_backward_sums R %d form %d' % case, worst)


@pytest.mark.parametrize('O', (128, 384))
def test_bn_fold_matches_float64(O):
    H = 1024
    worst = {}
    d = kr.bn_inputs(2, O, 'fold')
    for family in ('unit', 'exact'):
        if family == 'unit':
            S, W1, db1, g, b = kr.rnd('fold.S.%d' % O, (H, O)), kr.rnd('fold.W.%d' % O, (H, O), 0.05), kr.rnd('fold.db', (H,)), d['gamma'], d['beta']
        else:
            S, W1, db1 = kr.ints('fold.Si.%d' % O, (H, O), -4, 4), kr.ints('fold.Wi.%d' % O, (H, O), -2, 2), kr.ints('fold.dbi', (H,), -4, 4)
            g, b = kr.ints('fold.gi.%d' % O, (O,), -2, 2), kr.ints('fold.bi.%d' % O, (O,), -2, 2)
        Wd, dbd, gd, bd = dev(W1), dev(db1), dev(g), dev(b)

        def run():
            sdw, dg, db = Out(H, O, 'S / dW1', init=S), Out(1, O, 'dgamma'), Out(1, O, 'dbeta')
            _lib.check(L().pvr_op_policy_bn_fold(sdw.ptr, vp(Wd), vp(dbd), vp(gd), vp(bd), dg.ptr, db.ptr, H, O, st()))
            return dict(dW=sdw.read(), dgamma=dg.read(), dbeta=db.read())
        got = twice(run, 'bn_fold O %d' % O)
        for k, refb in zip(('dW', 'dgamma', 'dbeta'), kr.bn_fold_ref(S, W1, db1, g, b)):
            worst_of(worst, '%s/%s' % (family, k), chk(got[k], refb, 'bn_fold %s O %d' % (k, O), exact=family == 'exact'))
    o = Out(1, 72, 'refused bn_fold')
    assert L().pvr_op_policy_bn_fold(o.ptr, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr, H, 72, st()) == 1 and 'multiple of 128' in _lib.last_error()
    report('bn_fold O %d' % O, worst)


@pytest.mark.parametrize('R_', (1, 3, 130))
def test_bn_elementwise_kernels_match_float64(R_):
    worst = {}
    for Cc in (4, 72, 128):
        d = kr.bn_inputs(R_, Cc)
        dd = {k: dev(v) for k, v in d.items()}
        tag = 'R %d C %d' % (R_, Cc)

        def run():
            y0, y1, xh, dx = (Out(R_, Cc, w) for w in ('bn_apply', 'bn_apply eval', 'bn_xhat', 'bn_dx'))
            _lib.check(L().pvr_op_policy_bn_apply(vp(dd['x']), vp(dd['mean']), vp(dd['invstd']), vp(dd['gamma']), vp(dd['beta']), y0.ptr, R_, Cc, 0, st()))
            _lib.check(L().pvr_op_policy_bn_apply(vp(dd['x']), vp(dd['mean']), vp(dd['var']), vp(dd['gamma']), vp(dd['beta']), y1.ptr, R_, Cc, 1, st()))
            _lib.check(L().pvr_op_policy_bn_xhat(vp(dd['x']), vp(dd['mean']), vp(dd['invstd']), xh.ptr, R_, Cc, st()))
            _lib.check(L().pvr_op_policy_bn_dx(vp(dd['x']), vp(dd['dy']), vp(dd['mean']), vp(dd['invstd']), vp(dd['gamma']), vp(dd['dgamma']), vp(dd['dbeta']),
                                               dx.ptr, R_, Cc, 2 * R_, st()))
            res = dict(y0=y0.read(), y1=y1.read(), xhat=xh.read(), dx=dx.read())
            inplace = Out(R_, Cc, 'bn_dx_xhat', init=d['dy'])                   # in place on dy, from the xhat the kernel above wrote
            _lib.check(L().pvr_op_policy_bn_dx_xhat(inplace.ptr, vp(dev(res['xhat'])), vp(dd['invstd']), vp(dd['gamma']), vp(dd['dgamma']), vp(dd['dbeta']),
                                                    R_, Cc, 2 * R_, st()))
            res['dx_xhat'] = inplace.read()
            return res
        got = twice(run, 'bn elementwise ' + tag)
        x, m, s, g, b = (d[k] for k in ('x', 'mean', 'invstd', 'gamma', 'beta'))
        worst_of(worst, 'apply', chk(got['y0'], kr.bn_apply_ref(x, m, s, g, b, 0), 'bn_apply ' + tag))
        worst_of(worst, 'apply_eval', chk(got['y1'], kr.bn_apply_ref(x, m, d['var'], g, b, 1), 'bn_apply eval ' + tag))
        worst_of(worst, 'xhat', chk(got['xhat'], kr.bn_xhat_ref(x, m, s), 'bn_xhat ' + tag))
        worst_of(worst, 'dx', chk(got['dx'], kr.bn_dx_ref(d['dy'], g, s, d['dgamma'], d['dbeta'], 2 * R_, x=x, mean=m), 'bn_dx ' + tag))
        worst_of(worst, 'dx_xhat', chk(got['dx_xhat'], kr.bn_dx_ref(d['dy'], g, s, d['dgamma'], d['dbeta'], 2 * R_, xhat=got['xhat']), 'bn_dx_xhat ' + tag))
    report('bn elementwise R %d' % R_, worst)


# ------------------------------------------------------------------------------------------------------------------
# notdone, hprev, dlogits_pad (bit for bit), loss_mean
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tb', ((1, 1), (3, 5), (2, 33)), ids=str)
def test_small_kernels_bit_for_bit(tb):
    T, B = tb
    H, N = 1024, T * B
    done = (torch.arange(N) % 3 == 1).to(torch.uint8) * torch.tensor([1, 2, 255], dtype=torch.uint8).repeat(N)[:N]
    done[0], done[N - 1] = 7, 0
    hs, h0 = kr.rnd('hp.hs.%d.%d' % tb, (T, B, H)), kr.rnd('hp.h0.%d.%d' % tb, (B, H))
    nd = kr.notdone_ref(done).view(T, B)
    dd, hsd, h0d, ndd = dev(done), dev(hs), dev(h0), dev(nd)
    ndr = dev(kr.rnd('hp.nd.%d.%d' % tb, (T, B)))                                # a general factor: the product is still one rounding
    for A in (1, 3, 16):
        x = kr.rnd('pad.%d.%d' % (N, A), (N, A))
        xd = dev(x)

        def run():
            o_nd, o_hp, o_hp2, o_pad = Out(1, N, 'notdone'), Out(N, H, 'hprev'), Out(N, H, 'hprev general nd'), Out(N, 16, 'dlogits_pad')
            _lib.check(L().pvr_op_policy_notdone(vp(dd), o_nd.ptr, N, st()))
            _lib.check(L().pvr_op_policy_hprev(vp(hsd), vp(h0d), vp(ndd), o_hp.ptr, T, B, H, st()))
            _lib.check(L().pvr_op_policy_hprev(vp(hsd), vp(h0d), vp(ndr), o_hp2.ptr, T, B, H, st()))
            _lib.check(L().pvr_op_policy_dlogits_pad(vp(xd), o_pad.ptr, N, A, st()))
            return dict(nd=o_nd.read(), hprev=o_hp.read(), hprev2=o_hp2.read(), pad=o_pad.read())
        got = twice(run, 'small kernels %s' % (tb,))
        assert kr.bits_equal(got['nd'].view(T, B), nd), 'notdone'
        assert kr.bits_equal(got['hprev'].view(T, B, H), kr.hprev_ref(hs, h0, nd)), 'hprev'
        assert kr.bits_equal(got['hprev2'].view(T, B, H), kr.hprev_ref(hs, h0, ndr.cpu())), 'hprev with a general factor'
        assert kr.bits_equal(got['pad'], kr.dlogits_pad_ref(x)), 'dlogits_pad'
        assert all(torch.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize('n', (1, 255, 256, 257, 513))
def test_loss_mean_matches_float64(n):
    worst = {}
    for family, x in (('unit', kr.rnd('lm.%d' % n, (n,)).abs()), ('exact', kr.ints('lmi.%d' % n, (n,), 0, 7) * n)):
        xd = dev(x)

        def run():
            o = Out(1, 1, 'loss_mean')
            _lib.check(L().pvr_op_policy_loss_mean(vp(xd), n, o.ptr, st()))
            return dict(mean=o.read())
        got = twice(run, 'loss_mean %d' % n)
        worst_of(worst, family, chk(got['mean'], kr.loss_mean_ref(x), 'loss_mean %d %s' % (n, family)))
    report('loss_mean %d' % n, worst)


# ------------------------------------------------------------------------------------------------------------------
# LSTM steps
# ------------------------------------------------------------------------------------------------------------------
_wcache = {}


def lstm_w(H):
    if H not in _wcache:
        W, b = kr.lstm_weights(H)
        _wcache[H] = (W, b, dev(W), dev(b))
    return _wcache[H]


def _fwd_step(G, h, c, nd, Wd, bd, Bn, H):
    hd, cd, ndd = dev(h), dev(c), dev(nd)

    def run():
        g, ho, co = Out(Bn, 4 * H, 'G', init=G), Out(Bn, H, 'h_out'), Out(Bn, H, 'c_out')
        _lib.check(L().pvr_op_policy_lstm_fwd_step(g.ptr, vp(hd), vp(cd), vp(ndd), vp(Wd), vp(bd), ho.ptr, co.ptr, Bn, H, st()))
        return dict(gates=g.read(), h=ho.read(), c=co.read())
    return twice(run, 'lstm_fwd_step B %d H %d' % (Bn, H))


LSTM_SHAPES = [(1024, b) for b in (1, 15, 16, 17, 33, 64)] + [(2048, 1), (2048, 17)]


@pytest.mark.parametrize('case', LSTM_SHAPES, ids=lambda c: 'H%d_B%d' % c)
def test_lstm_fwd_step_matches_float64(case):
    H, Bn = case
    W, b, Wd, bd = lstm_w(H)
    worst = {}
    for family in kr.LSTM_FAMILIES:
        G, h, c, nd = kr.lstm_fwd_inputs(family, Bn, H)
        got = _fwd_step(G, h, c, nd, Wd, bd, Bn, H)
        for k, refb in kr.lstm_fwd_ref(G, h, c, nd, W, b).items():
            worst_of(worst, '%s/%s' % (family, k), chk(got[k], refb, 'lstm_fwd %s %s %s' % (case, family, k)))
    report('lstm_fwd_step H %d B %d' % case, worst)


def _bwd_step(d, Wd, Bn, H, has_next):
    dd = {k: dev(v) for k, v in d.items()}

    def run():
        g, dc, part = Out(Bn, 4 * H, 'gates / dG', init=d['gates']), Out(Bn, H, 'dc_carry', init=d['dc_carry']), Out(16 * Bn, H, 'partial')
        if has_next:
            s = L().pvr_op_policy_lstm_bwd_step(vp(dd['dG_next']), vp(Wd), vp(dd['nd_next']), vp(dd['dh_ext']), dc.ptr, g.ptr, vp(dd['c_t']), vp(dd['c_prev']),
                                                vp(dd['nd']), part.ptr, Bn, H, st())
        else:
            s = L().pvr_op_policy_lstm_bwd_step(None, None, None, vp(dd['dh_ext']), dc.ptr, g.ptr, vp(dd['c_t']), vp(dd['c_prev']), vp(dd['nd']), None, Bn, H, st())
        _lib.check(s)
        p = part.read()
        assert torch.isnan(p).all() if not has_next else torch.isfinite(p).all(), 'the partial buffer of the recurrent product'
        return dict(dG=g.read(), dc=dc.read())
    return twice(run, 'lstm_bwd_step B %d H %d next %d' % (Bn, H, has_next))


@pytest.mark.parametrize('case', LSTM_SHAPES, ids=lambda c: 'H%d_B%d' % c)
def test_lstm_bwd_step_matches_float64(case):
    H, Bn = case
    W, _, Wd, _ = lstm_w(H)
    worst = {}
    for family in kr.LSTM_FAMILIES:
        d = kr.lstm_bwd_inputs(family, Bn, H)
        for has_next in (True, False):
            got = _bwd_step(d, Wd, Bn, H, has_next)
            kw = dict(dc_carry=d['dc_carry'], dG_next=d['dG_next'], W_hh=W, nd_next=d['nd_next']) if has_next else {}
            ref = kr.lstm_bwd_ref(d['gates'], d['c_t'], d['c_prev'], d['nd'], d['dh_ext'], **kw)
            for k in ('dG', 'dc'):
                worst_of(worst, '%s/%s/next%d' % (family, k, has_next), chk(got[k], ref[k], 'lstm_bwd %s %s %s' % (case, family, k)))
            if family == 'impulse' and has_next:                                # one row of W_hh, bit for bit, in dc and in the candidate-gate block of dG
                row = W[d['dG_next'].argmax(1)]
                assert kr.bits_equal(got['dc'], row) and kr.bits_equal(got['dG'][:, 2 * H:3 * H].contiguous(), row), 'impulse: not the weight row'
                assert (got['dG'][:, :2 * H] == 0).all() and (got['dG'][:, 3 * H:] == 0).all()
    report('lstm_bwd_step H %d B %d' % case, worst)


def test_lstm_chain_of_three_steps_matches_float64_chain():
    """T = 3 through the entry points, each step fed with the previous step's own fp32 outputs, against the float64 chain fed with its own: the bounds
    on h and c (forward), on dG and dc (backward) are handed from step to step.  The backward chain takes the forward chain's fp32 activations as its
    inputs (they are inputs of those kernels), so what it carries is the error of dG_next and dc_carry."""
    T, Bn, H = 3, 5, 1024
    W, b, Wd, bd = lstm_w(H)
    nd = torch.ones(T, Bn)
    nd[1, 0] = nd[2, 4] = nd[1, 2] = 0.0
    Gx = kr.rnd('chain.G', (T, Bn, 4 * H))
    dh_ext = kr.rnd('chain.dh', (T, Bn, H), 1e-2)
    worst = {}
    h = c = torch.zeros(Bn, H)
    h64 = c64 = torch.zeros(Bn, H, dtype=torch.float64)
    e_h = e_c = torch.zeros(Bn, H, dtype=torch.float64)
    gates, cs = [], []
    for t in range(T):
        got = _fwd_step(Gx[t], h, c, nd[t], Wd, bd, Bn, H)
        ref = kr.lstm_fwd_ref(Gx[t], h64, c64, nd[t], W, b, e_h=e_h, e_c=e_c)
        for k in ('gates', 'h', 'c'):
            worst_of(worst, 'fwd/%s/t%d' % (k, t), chk(got[k], ref[k], 'chain forward t %d %s' % (t, k)))
        h, c, (h64, e_h), (c64, e_c) = got['h'], got['c'], ref['h'], ref['c']
        gates.append(got['gates']); cs.append(got['c'])
    dG_next = dc = dG64 = dc64 = e_dG = e_dc = None
    for t in range(T - 1, -1, -1):
        d = dict(gates=gates[t], c_t=cs[t], c_prev=cs[t - 1] if t else torch.zeros(Bn, H), nd=nd[t], dh_ext=dh_ext[t],
                 dc_carry=dc if dc is not None else torch.full((Bn, H), float('nan')), dG_next=dG_next if dG_next is not None else torch.zeros(Bn, 4 * H),
                 nd_next=nd[t + 1] if t < T - 1 else torch.ones(Bn))
        got = _bwd_step(d, Wd, Bn, H, t < T - 1)                                # (the last step's dc_carry holds NaN: it must not be read)
        kw = dict(dc_carry=dc64, dG_next=dG64, W_hh=W, nd_next=nd[t + 1], e_dG=e_dG, e_dc=e_dc) if t < T - 1 else {}
        ref = kr.lstm_bwd_ref(d['gates'], d['c_t'], d['c_prev'], d['nd'], d['dh_ext'], **kw)
        for k in ('dG', 'dc'):
            worst_of(worst, 'bwd/%s/t%d' % (k, t), chk(got[k], ref[k], 'chain backward t %d %s' % (t, k)))
        dG_next, dc, (dG64, e_dG), (dc64, e_dc) = got['dG'], got['dc'], ref['dG'], ref['dc']
    report('lstm chain T 3', worst)


# ------------------------------------------------------------------------------------------------------------------
# heads, heads backward
# ------------------------------------------------------------------------------------------------------------------
def _heads(x, Wp, bp, Wb, bb, tg, N, H, A):
    xd, Wpd, bpd, Wbd, bbd, tgd = (dev(v) for v in (x, Wp, bp, Wb, bb, tg))

    def run():
        lo, ba, ac = Out(N, A, 'logits'), Out(1, N, 'baseline'), Out(1, N, 'action', dtype=torch.int64)
        lr, dl = Out(1, N, 'loss_row'), Out(N, 16, 'dlogits')
        _lib.check(L().pvr_op_policy_heads(vp(xd), vp(Wpd), vp(bpd), vp(Wbd), vp(bbd), vp(tgd), lo.ptr, ba.ptr, ac.ptr, lr.ptr if tg is not None else None,
                                           dl.ptr if tg is not None else None, N, H, A, st()))
        res = dict(logits=lo.read(), baseline=ba.read().view(N), action=ac.read().view(N), loss_row=lr.read().view(N), dlogits=dl.read())
        if tg is None:
            assert torch.isnan(res['loss_row']).all() and torch.isnan(res['dlogits']).all(), 'without a target nothing may be written there'
            del res['loss_row'], res['dlogits']
        return res
    return twice(run, 'heads N %d H %d A %d' % (N, H, A))


@pytest.mark.parametrize('A', (1, 3, 16))
@pytest.mark.parametrize('H', (1024, 2048))
def test_heads_match_float64(H, A):
    worst = {}
    for N in (1, 3, 4, 5, 9):
        for family in kr.HEADS_FAMILIES:
            x, Wp, bp, Wb, bb, tg = kr.heads_inputs(family, N, H, A)
            for with_target in (True, False):
                what = 'heads N %d H %d A %d %s target %d' % (N, H, A, family, with_target)
                got = _heads(x, Wp, bp, Wb, bb, tg if with_target else None, N, H, A)
                ref = kr.heads_ref(x, Wp, bp, Wb, bb, tg if with_target else None)
                for k in ('logits', 'baseline') + (('loss_row', 'dlogits') if with_target else ()):
                    worst_of(worst, '%s/%s' % (family, k), chk(got[k], ref[k], what + ' ' + k, exact=family != 'unit' and k in ('logits', 'baseline')))
                assert torch.equal(got['action'], kr.first_argmax(got['logits'])), what + ': the action is not the first maximum of the logits'
                if with_target:
                    assert (got['dlogits'][:, A:] == 0).all() and not torch.signbit(got['dlogits'][:, A:]).any(), what + ': padding columns'
                if family == 'exact' and A >= 3:
                    l = got['logits']
                    assert (l[:, 1] == l[:, 2]).all() and (got['action'] != 2).all(), what + ': a tie must give the first index'
                    if A == 3:
                        assert (got['action'] == 1).all()
    report('heads H %d A %d' % (H, A), worst)


@pytest.mark.parametrize('A', (1, 3, 16))
def test_heads_target_out_of_range_gives_nan_on_that_row_only(A):
    N, H = 9, 1024
    x, Wp, bp, Wb, bb, tg = kr.heads_inputs('unit', N, H, A)
    tg = tg.clone()
    tg[0], tg[4], tg[8] = -1, A, 1 << 40
    got = _heads(x, Wp, bp, Wb, bb, tg, N, H, A)
    ref = kr.heads_ref(x, Wp, bp, Wb, bb, tg)
    bad = ~ref['target_ok']
    assert int(bad.sum()) == 3 and torch.isnan(got['loss_row'][bad]).all() and torch.isfinite(got['loss_row'][~bad]).all()
    assert torch.isfinite(got['dlogits']).all() and torch.isfinite(got['logits']).all()
    worst = {k: kr.ratio(got[k][~bad], ref[k][0][~bad], ref[k][1][~bad]) for k in ('loss_row', 'dlogits', 'logits')}
    report('heads bad targets A %d' % A, worst)


HB_CASES = [(n, a, 1024, f) for n in (1, 9, 65) for a in (1, 3, 16) for f in (0, 1)] + [(n, a, 1024, -1) for n in BOUNDARY for a in (1, 3, 16)] + \
           [(9, 3, 2048, 0), (9, 3, 2048, 1), (513, 3, 2048, -1)]


@pytest.mark.parametrize('case', HB_CASES, ids=lambda c: 'N%d_A%d_H%d_form%d' % c)
def test_head_backward_matches_float64(case):
    N, A, H, form = case
    worst = {}
    for family in kr.REDUCE_FAMILIES:
        dl, x, Wp = kr.head_backward_inputs(family, N, H, A)
        dld, xd, Wd = dev(dl), dev(x), dev(Wp)

        def run():
            dW, db, dout = Out(A, H, 'dWp'), Out(1, A, 'dbp'), Out(N, H, 'dout')
            before = L().pvr_debug_policy_two_stage_launches()
            _lib.check(L().pvr_op_policy_head_backward(vp(dld), vp(xd), vp(Wd), dW.ptr, db.ptr, dout.ptr, N, H, A, form, st()))
            run.form = expect_form(form, N, True, before)
            return dict(dWp=dW.read(), dbp=db.read(), dout=dout.read())
        got = twice(run, 'head_backward %s %s' % (case, family))
        for k, refb in zip(('dWp', 'dbp', 'dout'), kr.head_backward_ref(dl, x, Wp, run.form)):
            worst_of(worst, '%s/%s' % (family, k), chk(got[k], refb, 'head_backward %s %s %s' % (case, family, k), exact=family != 'unit'))
    report('head_backward N %d A %d H %d form %d' % case, worst)


# ------------------------------------------------------------------------------------------------------------------
# masked GEMM
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ((0, 0), (0, 1), (1, 1)), ids=lambda l: 'akm%d_bkn%d' % l)
@pytest.mark.parametrize('shape', ((100, 64, 32), (37, 1024, 1024), (64, 64, 4096)), ids=lambda s: 'x'.join(str(v) for v in s))
def test_gemm_masked_matches_float64(shape, layout):
    Mm, N, K = shape
    a_km, b_kn = layout
    A_, B_, bias, mask = kr.gemm_inputs(Mm, N, K)
    Ad, Bd = dev(A_.t() if a_km else A_), dev(B_.t() if b_kn else B_)          # storage [K][M] / [K][N] when the flag is set
    md, biasd = dev(mask), dev(bias)
    worst = {}
    if a_km and Mm % 4:
        o = Out(Mm, N, 'refused gemm')
        assert L().pvr_op_gemm_f32_masked(vp(Ad), vp(Bd), None, vp(md), o.ptr, Mm, N, K, a_km, b_kn, 0, st()) == 1 and 'multiples of 4' in _lib.last_error()
        assert torch.isnan(o.read()).all()
        return
    for use_bias, relu, use_mask in ((0, 0, 1), (1, 1, 1), (1, 0, 0)):

        def run():
            o = Out(Mm, N, 'gemm C')
            _lib.check(L().pvr_op_gemm_f32_masked(vp(Ad), vp(Bd), vp(biasd) if use_bias else None, vp(md) if use_mask else None, o.ptr, Mm, N, K, a_km, b_kn,
                                                  relu, st()))
            return dict(C=o.read())
        got = twice(run, 'gemm %s %s' % (shape, layout))['C']
        ref, bound, zero = kr.gemm_masked_ref(A_, B_, bias if use_bias else None, mask if use_mask else None, relu)
        worst_of(worst, 'bias%d_relu%d_mask%d' % (use_bias, relu, use_mask), chk(got, (ref, bound), 'gemm %s %s' % (shape, layout)))
        assert (got[zero] == 0).all(), 'an element whose mask is <= 0 is not zero'
        if not relu:
            assert (got[~zero] != 0).all(), 'an element whose mask is > 0 came out zero'
    report('gemm_masked %s splits %d layout %s' % (shape, kr.gemm_splits(Mm, N, K), layout), worst)


# ------------------------------------------------------------------------------------------------------------------
# clip + RMSprop over several buffers
# ------------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=f32(1e-3), alpha=f32(0.99), eps=f32(1e-5))


def _rmsprop(P, V, G, max_norm, with_stats):
    gd = [dev(g) for g in G]
    arr = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)

    def run():
        ps = [Out(1, p.numel(), 'params %d' % i, init=p) for i, p in enumerate(P)]
        vs = [Out(1, v.numel(), 'square_avg %d' % i, init=v) for i, v in enumerate(V)]
        stat = Out(1, 1, 'stats_out')
        counts = (C.c_int64 * len(P))(*[p.numel() for p in P])
        _lib.check(L().pvr_joint_apply_rmsprop(len(P), arr([o.ptr.value for o in ps]), arr([o.ptr.value for o in vs]), arr([g.data_ptr() for g in gd]), counts,
                                               HYPER['lr'], HYPER['alpha'], HYPER['eps'], max_norm, stat.ptr if with_stats else None, st()))
        res = {'p%d' % i: o.read() for i, o in enumerate(ps)}
        res.update({'v%d' % i: o.read() for i, o in enumerate(vs)})
        res['norm'] = stat.read()
        return res
    return twice(run, 'joint rmsprop')


@pytest.mark.parametrize('counts', ((4,), (1020,), (1024,), (4100,), (1048580,), (4, 1020, 4100), (1024, 1048580, 4)), ids=str)
def test_joint_apply_rmsprop_matches_float64(counts):
    worst = {}
    for scale in (1.0, 1e-5):
        P, V, G = kr.rmsprop_inputs(counts, scale)
        norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in G)))
        for side, mn in (('unclipped', f32(norm * 4)), ('clipped', f32(norm / 4))):
            (rn, bn), ps, vs = kr.rmsprop_ref(P, V, G, max_norm=mn, **HYPER)
            for with_stats in (True, False):
                got = _rmsprop(P, V, G, mn, with_stats)
                if with_stats:
                    worst_of(worst, side + '/norm', chk(got['norm'].view(()), (rn, bn), 'norm %s' % (counts,)))
                else:
                    assert torch.isnan(got['norm']).all(), 'stats_out == NULL: nothing to write'
                for k in range(len(counts)):
                    worst_of(worst, side + '/p', chk(got['p%d' % k], ps[k], 'params %s group %d' % (counts, k)))
                    worst_of(worst, side + '/v', chk(got['v%d' % k], vs[k], 'square_avg %s group %d' % (counts, k)))
    report('joint rmsprop %s' % (counts,), worst)


# ------------------------------------------------------------------------------------------------------------------
# whole steps at the 512-row dispatch boundary: 510, 512 and twice 513 rows; B in the second, third and fourth 16-row group, a ragged last chunk
# ------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(T, B, O, 1) for (T, B) in ((17, 30), (8, 64), (27, 19), (9, 57)) for O in (72, 128)]
_step_refs = {}


def step_refs(case):
    if case not in _step_refs:
        T, B, O, bn = case
        sd = R.policy_params(7, O, bn)
        obs, done, act = R.inputs(11 + O, T, B, O)
        _step_refs[case] = dict(sd=sd, obs=obs, done=done, act=act, f64=R.dobs_autograd(sd, obs, done, act, bn, torch.float64),
                                f32=R.dobs_autograd(sd, obs, done, act, bn, torch.float32))
    return _step_refs[case]


def _policy(case, train):
    T, B, O, bn = case
    m = M.PolicyNet((O,), R.A, bool(bn), max_unroll=T, max_batch=B)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in step_refs(case)['sd'].items()})
    m = m.to(device='cuda')
    m.train(train)
    m._ensure(T, B)
    return m


@pytest.mark.parametrize('case', STEP_CASES, ids=str)
def test_every_gradient_tensor_at_the_dispatch_boundary(case):
    """Regression test of heads_kernel's softmax.  With p = expf(l - lse), lse = mx + logf(se), the probabilities of a row added up to 1 + 3e-08 on
    average (a bias of the library functions, inside the elementwise bound), and d(loss)/d(policy.bias) sums that over all rows: 4.2e-07 ... 4.7e-07 from
    float64 at every shape here, 8.28 x torch fp32's distance at (27, 19, 72, 1).  The kernel now normalises by division, p = expf(l - mx) / se; the
    same figure is 0.33 ... 0.84 x torch's."""
    T, B, O, bn = case
    r = step_refs(case)
    m = _policy(case, True)
    x = torch.flatten(r['obs'], 0, 1).cuda().contiguous()
    d, a = r['done'].to(torch.uint8).cuda(), r['act'].cuda()
    bns = m._bn_struct()
    before = L().pvr_debug_policy_two_stage_launches()
    runs = []
    for _ in range(2):
        g = torch.full((m._n_train,), float('nan'), device='cuda')
        _lib.check(L().pvr_policy_backward(m._handle, vp(m._flat), C.byref(bns) if bns else None, vp(x), vp(d), vp(a), T, B, vp(g), None, None, st()))
        torch.cuda.synchronize()
        runs.append(g.cpu())
    took = L().pvr_debug_policy_two_stage_launches() - before
    assert (took > 0) == (T * B >= 512), 'T * B = %d rows: %d two-stage reductions' % (T * B, took)
    worst, failed = {}, {}
    for k, (o, shp) in m._slots.items():
        if o >= m._n_train:
            continue
        n = int(np.prod(shp))
        got = runs[0][o:o + n].view(shp)
        assert torch.isfinite(got).all(), k
        assert kr.bits_equal(got, runs[1][o:o + n].view(shp)), '%s: two runs differ' % k
        ok, dist, d32 = R.accept(got, r['f32'][1][k], r['f64'][1][k])
        worst[k] = dist / d32
        if not ok:
            failed[k] = (dist, d32)
    m.close()
    print('\n[gradients %s] rel-L2 to float64 over torch fp32\'s: %s' % (case, {k: '%.2f' % v for k, v in sorted(worst.items())}))
    assert not failed, failed


@pytest.mark.parametrize('case', STEP_CASES, ids=str)
def test_eval_forward_with_carried_state_at_the_dispatch_boundary(case):
    T, B, O, bn = case
    r = step_refs(case)
    m = _policy(case, False)
    H = R.HIDDEN
    h0, c0 = 0.5 * kr.rnd('step.h0.%d' % B, (2, B, H)), 0.5 * kr.rnd('step.c0.%d' % B, (2, B, H))
    rm, rv = 1.0 + 0.1 * kr.rnd('step.rm.%d' % O, (O,)), 0.5 + kr.rnd('step.rv.%d' % O, (O,)).abs()
    m.load_state_dict({'fc.0.running_mean': rm, 'fc.0.running_var': rv}, strict=False)
    outs = {}
    for dt in (torch.float64, torch.float32):
        p = R.to_dtype(r['sd'], dt)
        with torch.no_grad():
            outs[dt] = kr.eval_forward(p, r['obs'].to(dt), r['done'], h0.to(dt), c0.to(dt), bn, rm.to(dt), rv.to(dt))
    x = torch.flatten(r['obs'], 0, 1).cuda().contiguous()
    d = r['done'].to(torch.uint8).cuda()
    got = [tuple(t.cpu() for t in m._forward_raw(x, d, h0.cuda(), c0.cuda(), T, B, False)) for _ in range(2)]
    m.close()
    worst = {}
    for i, name in ((0, 'logits'), (1, 'baseline'), (3, 'h'), (4, 'c')):
        j = {0: 0, 1: 1, 3: 2, 4: 3}[i]
        g = got[0][i].reshape(outs[torch.float64][j].shape)
        assert torch.isfinite(g).all() and kr.bits_equal(got[0][i], got[1][i]), name
        ok, dist, d32 = R.accept(g, outs[torch.float32][j], outs[torch.float64][j])
        worst[name] = dist / d32
        assert ok, (name, dist, d32)
    print('\n[eval forward %s] rel-L2 to float64 over torch fp32\'s: %s' % (case, {k: '%.2f' % v for k, v in sorted(worst.items())}))
