"""GPU: every attention kernel of the CLIP towers (csrc/clip.hip) on its own against an f64 softmax, on PEAKED inputs.

`ssw_debug_attention_run` / `ssw_debug_skinny_attn_out_run` (lab build, include/seesaw_hip_debug.h) run ONE launch of
one kernel with its production launch shape on operands the test supplies:

    form 0 attention_mfma<4>    1 attention_mfma<4, 2>    2 attention_mfma<5>    3 attention_rows64
    form 4 launch_attention_long (attention_long<4 / 5 / 13 / 17>)    5 attn_pooled_rows    skinny_attn_out<1 / 2>

and the fused image launch (csrc/attn_out.hip) takes the same inputs through `ssw_debug_attn_out_run`.  The towers'
own tests carry random-init weights: their attention logits are ~0.04, every softmax is uniform to three digits, and a
missing max-subtraction, a mask off by one, a clamped key row that leaks or a swizzle that permutes keys inside a tile
changes nothing a tolerance can see.  Here the softmax has a few dominant keys, as a trained CLIP's has.

The reference is numpy float64 over the same bf16-valued operands: softmax(scale q k^T + mask) v per (sequence, head).

Every launch: B = 3 sequences (8 for the pooled row) and the model's H; >= 32 guard rows of bf16 NaN (0x7FC0) behind
the qkv rows; the out buffer, 16 guard rows included, prefilled with a NaN sentinel pattern.  The output must be finite
and every guard row must come back untouched: an over-read shows as NaN, an over-write as a changed guard, an
unwritten row as its sentinel -- none of them can fault.  (The skinny hook keeps its guards on the device: 32 rows of
0xFF behind qkv, residual and out; a write into them is its error.)

Input families (all values exact in bf16, seeds fixed)
  (a) one-hot, BIT-EXACT.  Keys are distinct +-1 sign vectors of 64 dims whose pairwise dot products are <= 32 (drawn
      greedily, seed 1), query i = 8 key t(i), V integer-valued in [-8, 8] without 0.  With scale 1/8 the target's logit
      is 64 and every other <= 32.  CONDITION, asserted from the f64 reference before every launch: the target's weight is
      >= 1 - 2^-20.  Then bf16(P) is one-hot up to stray columns of <= e^-32, the f32 sum differs from V[t(i)] by
      <= 272 * 8 * e^-32 ~ 3e-11, far inside half a bf16 ulp of a value of magnitude >= 1 (why V avoids 0: a zero would
      come back as that stray mass, not as a zero), and the stored row must be V[t(i)] bit for bit.
      t(i) = (i + s) mod S non-causal, max(0, i - s) causal, s in {0, 1, 15, 16, 17, S - 1}.
  (b) two-hot, BIT-EXACT (non-causal).  Key row S - 1 is a copy of key row 0 (second variant: key 16 of key 15) and every
      query aims at it: both logits are the same f32, P = (1/2, 1/2), and 0.5 (V[a] + V[b]) -- an integer or a half
      below 8.5 in magnitude, exact in bf16, and nonzero by construction -- must come back bit for bit.  A clamped key
      row counted twice gives 2/3, 1/3.
  (c) needle behind the mask (causal; block-causal for the skinny kernel): query i = 8 key t(i) with t(i) in the
      query's masked future -- the very next key for even i -- or, for the skinny kernel, in another sequence of the
      call.  The reference spreads over the allowed keys only; a leak puts all the mass on the needle.
  (d) peaked random: q, k ~ N(0, 2^2) rounded to bf16, v ~ N(0, 1).  Checked on the CPU
      (test_peaked_inputs_and_tolerance_on_the_cpu, which needs no GPU): logit std 4 +- 0.3, median top weight of a
      row within 0.45 .. 0.8 for S in 17 .. 272.
  (e) offset: (d) with q[:, 63] = 16 and k[:, 63] = 50, so every logit carries +100 and __expf overflows without the
      max-subtraction.

Tolerance for (c), (d), (e) -- derived, computed from the reference alone (u = 2^-8, bf16's unit roundoff):

    |got - ref| <= (1 + 2^-6) u (sum_j P_j |v_j| + |ref|)  +  f32 term

  bf16 term: the kernel rounds P once (|P^_j - P_j| <= u P_j, so the f32 product moves by <= u sum_j P_j |v_j|) and the
  output once more (<= u |o| <= u (|ref| + u sum P|v|)); (1 + 2^-6) covers the second-order part.
  f32 term, in the reference's quantities, with x_j = logit_j - max logit (<= 0):
    * a logit is a 64-term f32 sum of exact products, scaled: |d_j| <= 66 * 2^-24 * scale * sum_d |q_d| |k_d|;
    * the maximum cancels in the normalisation; the subtraction, the product with log2(e) and v_exp_f32 give the
      exponential a relative error <= |x_j| 2^-21 + 2^-22;  eps_j = d_j + |x_j| 2^-21 + 2^-22;
    * normalisation: N = sum_j P_j eps_j + (S + 4) 2^-24 (f32 sum, reciprocal, product);
    * the f32 accumulation of P^ V over <= 288 key slots: 288 * 2^-24 * (1 + 2^-7) sum_j P_j |v_j|;
    * exponentials below the f32 normal range flush: S * 2^-126 * max|v|.
    f32 term = 1.01 sum_j P_j (eps_j + N) |v_j| + 288 * 2^-24 (1 + 2^-7) sum_j P_j |v_j| + S 2^-126 max|v|
  CONDITION, asserted in every case the file runs: f32 term <= half the bf16 term, element by element.  Inputs that
  miss it are wrong inputs; the tolerance is not to be widened.  A numpy emulation of the kernel's rounding sequence
  (f32 logits, exp, normalise, bf16, f32 product, bf16) stays within the bound on the CPU (same CPU test).
  For the skinny kernel the attention tolerance is carried through the out-projection, sum_d tol[d] |Wo[n, d]|, plus
  the f32 product's own summation term, 520 * 2^-24 (sum_d (|ref_d| + tol_d) |Wo[n, d]| + |bias| + |residual|).

Same-bits claims (comments on attention_rows64, attention_long, attn_pooled_rows, attn_outproj_image), byte for byte on
(d) and (e): forms 0, 1, 3, 4 for every S <= 64; forms 2 and 4 for every S <= 80; form 5 = row 0 of form 3; the fused
image launch's rows = form 3's.
"""
import ctypes

import numpy as np
import pytest

gpu = pytest.mark.gpu

U = 2.0 ** -8
SCALE = 0.125
QKV_GUARD, OUT_GUARD = 32, 16
SHIFTS = (0, 1, 15, 16, 17, -1)  # -1 stands for S - 1
MAX_S = {0: 64, 1: 64, 2: 80, 3: 64, 4: 272, 5: 64}

_S64 = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 63, 64)
_S80 = (1, 16, 64, 65, 77, 79, 80)
_S272 = (1, 17, 64, 65, 80, 81, 82, 127, 128, 129, 197, 207, 208, 209, 225, 255, 256, 257, 271, 272)
FORM_SHAPES = {f: {(768, 12, s) for s in _S64} | {(d, h, s) for d, h in ((512, 8), (1024, 16)) for s in (1, 17, 50, 64)}
               for f in (0, 1, 3)}
FORM_SHAPES[2] = {(d, h, s) for d, h in ((512, 8), (768, 12)) for s in _S80}
FORM_SHAPES[4] = {(768, 12, s) for s in _S272} | {(1024, 16, s) for s in (81, 197, 257, 272)}
ALL_SHAPES = sorted(set().union(*FORM_SHAPES.values()))


# ---- bf16 <-> f32, bit patterns -------------------------------------------------------------------------------------
def _bits(x):
    """finite f32 values -> uint16 bit patterns of the round-to-nearest-even bf16"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)


def _vals(bits):
    return (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32)


def _round(x):
    return _vals(_bits(x))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _sentinel(shape):
    """bf16 NaN patterns 0x7FC1 .. 0x7FFD, varying along the buffer"""
    n = int(np.prod(shape))
    return (0x7FC1 + (np.arange(n, dtype=np.uint32) % 61)).astype(np.uint16).reshape(shape)


def _finite(bits):
    return bool(((bits & 0x7F80) != 0x7F80).all())


def _rows(x):
    """[B, H, S, 64] -> [B S, 64 H]"""
    B, H, S, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * S, H * 64)


def _pack(q, k, v):
    """q, k, v [B, H, S, 64] (bf16-valued f32) -> the fused rows [B S, 3 D] (q | k | v) as bit patterns"""
    for a in (q, k, v):
        assert np.array_equal(_round(a), a.astype(np.float32)), "operands must be exact in bf16"
    return _bits(np.concatenate([_rows(q), _rows(k), _rows(v)], axis=1))


# ---- the reference and the tolerance --------------------------------------------------------------------------------
def _allowed(S, causal, L=None):
    """[S, S] bool: may query i see key j; L: rows of several sequences of L share the tile (the skinny kernel)"""
    i, j = np.arange(S)[:, None], np.arange(S)[None, :]
    ok = np.ones((S, S), dtype=bool) if L is None else (i // L == j // L)
    return ok & (j <= i) if causal else ok


class Ref:
    """softmax(scale q k^T + mask) v in f64, and the two tolerance terms of the module docstring"""

    def __init__(self, q, k, v, allowed, tolerance=True):
        q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
        S = q.shape[2]
        logits = SCALE * (q64 @ k64.transpose(0, 1, 3, 2))
        logits = np.where(allowed, logits, -np.inf)
        x = logits - logits.max(axis=-1, keepdims=True)
        e = np.exp(x)
        self.P = P = e / e.sum(axis=-1, keepdims=True)
        if not tolerance:  # (the bit-exact families read P only)
            return
        self.ref = P @ v64
        apv = P @ np.abs(v64)
        self.bf_term = (1 + 2.0 ** -6) * U * (apv + np.abs(self.ref))
        d = 66 * 2.0 ** -24 * SCALE * (np.abs(q64) @ np.abs(k64).transpose(0, 1, 3, 2))
        eps = np.where(allowed, d + np.where(allowed, -x, 0.0) * 2.0 ** -21 + 2.0 ** -22, 0.0)
        N = (P * eps).sum(axis=-1, keepdims=True) + (S + 4) * 2.0 ** -24
        self.f32_term = (1.01 * ((P * (eps + N)) @ np.abs(v64)) + 288 * 2.0 ** -24 * (1 + 2.0 ** -7) * apv
                         + S * 2.0 ** -126 * np.abs(v64).max())
        self.tol = self.bf_term + self.f32_term

    def check_condition(self, what):
        assert (self.f32_term <= 0.5 * self.bf_term).all(), ("f32 term above half the bf16 term: wrong inputs", what,
                                                             float((self.f32_term / self.bf_term).max()))


def _assert_close(got_bits, r, what):
    """got_bits [B S, D] against the reference's rows, element by element"""
    got = _vals(got_bits).astype(np.float64)
    d, tol = np.abs(got - _rows(r.ref)), _rows(r.tol)
    worst = float((d / tol).max())
    print(f"{what}: max |got - ref| / tol = {worst:.3f}, max |got - ref| = {float(d.max()):.3e}")
    assert (d <= tol).all(), (what, worst, float(d.max()))


# ---- input families -------------------------------------------------------------------------------------------------
_SIGN_KEYS = None


def _sign_keys():
    """272 distinct +-1 vectors of 64 dims with pairwise dot products <= 32 (seed 1, rows redrawn until they fit)"""
    global _SIGN_KEYS
    if _SIGN_KEYS is None:
        rng = np.random.default_rng(1)
        keys = np.zeros((272, 64), dtype=np.float32)
        for i in range(272):
            while True:
                keys[i] = rng.choice(np.float32([-1, 1]), 64)
                if i == 0 or (keys[:i] @ keys[i]).max() <= 32:
                    break
        _SIGN_KEYS = keys
    return _SIGN_KEYS


def _keys(rng, B, H, S):
    """per (sequence, head): S of the sign keys in a random order with random column flips (dot products unchanged)"""
    base = _sign_keys()
    k = np.empty((B, H, S, 64), dtype=np.float32)
    for b in range(B):
        for h in range(H):
            k[b, h] = base[rng.permutation(272)[:S]] * rng.choice(np.float32([-1, 1]), 64)
    return k


def _aimed(k, target):
    """query i = 8 key target[..., i]; target [S] or [B, S]"""
    B, H, S, _ = k.shape
    t = np.broadcast_to(np.asarray(target), (B, S))
    return 8 * np.take_along_axis(k, np.broadcast_to(t[:, None, :, None], (B, H, S, 64)), axis=2)


def _int_values(rng, shape):
    return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


def one_hot(seed, B, H, S, target):
    rng = np.random.default_rng(seed)
    k = _keys(rng, B, H, S)
    return _aimed(k, target), k, _int_values(rng, (B, H, S, 64))


def two_hot(seed, B, H, S, a, b):
    """key row b a copy of key row a, every query aims at it; returns q, k, v and the expected row 0.5 (V[a] + V[b])"""
    rng = np.random.default_rng(seed)
    k = _keys(rng, B, H, S)
    k[:, :, b] = k[:, :, a]
    v = _int_values(rng, (B, H, S, 64))
    v[:, :, b] = np.where(v[:, :, a] + v[:, :, b] == 0, v[:, :, a], v[:, :, b])  # no zero in the expected row
    return _aimed(k, np.full(S, a)), k, v, 0.5 * (v[:, :, a] + v[:, :, b])


def needle(seed, B, H, S, target):
    rng = np.random.default_rng(seed)
    k = _keys(rng, B, H, S)
    return _aimed(k, target), k, _round(rng.standard_normal((B, H, S, 64)))


def peaked(seed, B, H, S, offset=False):
    rng = np.random.default_rng(seed)
    q, k = (_round(2 * rng.standard_normal((B, H, S, 64))) for _ in range(2))
    v = _round(rng.standard_normal((B, H, S, 64)))
    if offset:
        q[..., 63], k[..., 63] = 16, 50
    return q, k, v


def _shift_target(S, s, causal, L=None):
    """t(i) = (i + s) mod S non-causal, max(0, i - s) causal -- inside each sequence of L rows when L is given"""
    L = S if L is None else L
    i = np.arange(S)
    s = (L - 1 if s < 0 else s)
    pos = i % L
    return i - pos + (np.maximum(0, pos - s) if causal else (pos + s) % L)


def _future_target(S):
    """a key of the query's masked future: the next one for even i, the last one for odd i (the last query: itself)"""
    i = np.arange(S)
    return np.where(i == S - 1, i, np.where(i % 2 == 0, np.minimum(i + 1, S - 1), S - 1))


# ---- launches -------------------------------------------------------------------------------------------------------
def _launch(lib, form, q, k, v, causal):
    """one launch of `form`; returns the written rows [B S, D] ([B, D] for form 5) as bf16 bit patterns"""
    B, H, S, _ = q.shape
    D = 64 * H
    qkv = np.full((B * S + QKV_GUARD, 3 * D), 0x7FC0, dtype=np.uint16)
    qkv[:B * S] = _pack(q, k, v)
    n_out = B if form == 5 else B * S
    out = _sentinel((n_out + OUT_GUARD, D))
    before = out.copy()
    rc = lib.ssw_debug_attention_run(form, B, S, D, H, causal, SCALE, _p(qkv), qkv.shape[0], _p(out), out.shape[0])
    assert rc == 0, lib.ssw_last_error().decode()
    what = (form, B, S, D, causal)
    assert np.array_equal(out[n_out:], before[n_out:]), ("a guard row of the output was written", what)
    assert _finite(out[:n_out]), ("NaN / inf / an unwritten row in the output", what)
    return out[:n_out]


def _forms_for(D, H, S):
    return [f for f in sorted(FORM_SHAPES) if (D, H, S) in FORM_SHAPES[f]]


def _assert_one_hot(r, target, what, pair=None):
    """the one-hot condition, from the reference: the target (or the pair's two halves) holds >= 1 - 2^-20 of every row"""
    B, H, S, _ = r.P.shape
    t = np.broadcast_to(np.asarray(target), (B, S))[:, None, :, None]
    w = np.take_along_axis(r.P, np.broadcast_to(t, (B, H, S, 1)), axis=3)[..., 0]
    if pair is not None:
        w2 = r.P[..., pair]
        assert np.array_equal(w, w2), what
        w = w + w2
    assert (w >= 1 - 2.0 ** -20).all(), ("one-hot condition missed", what, float(w.min()))


@gpu
@pytest.mark.parametrize("D,H,S", ALL_SHAPES)
def test_each_kernel_against_the_f64_softmax(lab_build, D, H, S):
    """forms 0 .. 4 at the shapes that hit every edge of each (tile counts, the 64 / 80 / 208 thresholds of the instances,
    the 272 limit): families (a), (b) bit for bit, (c), (d), (e) within the derived tolerance, both masks; the forms that
    share a shape agree byte for byte"""
    lib, B = lab_build, 3
    forms = _forms_for(D, H, S)
    seed = 1000 * S + H

    def run_all(q, k, v, causal, check):
        """every form of this shape: each output against the expectation first, then against one another"""
        outs = [_launch(lib, f, q, k, v, causal) for f in forms]
        for f, o in zip(forms, outs):
            check(f, o)
        for f, o in zip(forms[1:], outs[1:]):
            assert np.array_equal(o, outs[0]), (f"forms {forms[0]} and {f} differ", D, S, causal)

    for causal in (0, 1):
        ok = _allowed(S, causal)
        for s in SHIFTS:                                                        # (a)
            t = _shift_target(S, s, causal)
            q, k, v = one_hot(seed + 10 + s, B, H, S, t)
            _assert_one_hot(Ref(q, k, v, ok, tolerance=False), t, ("a", D, S, causal, s))
            want = _bits(_rows(np.take_along_axis(v, np.broadcast_to(t[None, None, :, None], v.shape), axis=2)))

            def exact(f, got, want=want, s=s):
                assert np.array_equal(got, want), ("one-hot rows are not V[t(i)] bit for bit", f, D, S, causal, s,
                                                   int((got != want).any(axis=1).sum()))
            run_all(q, k, v, causal, exact)
        if not causal:                                                          # (b)
            for a, b in ((0, S - 1), (15, 16)):
                if b <= a or b >= S:
                    continue
                q, k, v, want = two_hot(seed + 20 + a, B, H, S, a, b)
                _assert_one_hot(Ref(q, k, v, ok, tolerance=False), np.full(S, a), ("b", D, S, a, b), pair=b)
                want = _bits(_rows(np.broadcast_to(want[:, :, None, :], v.shape)))

                def exact2(f, got, want=want, a=a, b=b):
                    assert np.array_equal(got, want), ("two-hot rows are not (V[a] + V[b]) / 2 bit for bit", f, D, S, a, b)
                run_all(q, k, v, causal, exact2)
        cases = [("d", peaked(seed + 30 + causal, B, H, S)), ("e", peaked(seed + 40 + causal, B, H, S, offset=True))]
        if causal:
            cases.append(("c", needle(seed + 50, B, H, S, _future_target(S))))
        for name, (q, k, v) in cases:                                           # (c), (d), (e)
            r = Ref(q, k, v, ok)
            r.check_condition((name, D, S, causal))
            run_all(q, k, v, causal, lambda f, got: _assert_close(got, r, f"family {name} form {f} D={D} S={S} causal={causal}"))


@gpu
@pytest.mark.parametrize("first", range(1, 81, 16))
def test_same_bits_at_every_length(lab_build, first):
    """the claims in the kernels' comments: attention_mfma<4>, <4, 2>, attention_rows64 and attention_long<4> leave the same
    bytes for every S <= 64, attention_mfma<5> and attention_long<4 / 5> for every S <= 80 -- on peaked and offset inputs,
    both masks"""
    lib, B, H = lab_build, 3, 12
    for S in range(first, first + 16):
        forms = [f for f in (0, 1, 2, 3, 4) if S <= MAX_S[f]]
        for causal in (0, 1):
            for offset in (False, True):
                q, k, v = peaked(5000 + 4 * S + 2 * causal + offset, B, H, S, offset)
                outs = [_launch(lib, f, q, k, v, causal) for f in forms]
                for f, o in zip(forms[1:], outs[1:]):
                    assert np.array_equal(o, outs[0]), (f"forms {forms[0]} and {f} differ", S, causal, offset)


@gpu
@pytest.mark.parametrize("S", [1, 8, 15, 16, 17, 33, 50, 63, 64])
def test_pooled_row_kernel(lab_build, S):
    """attn_pooled_rows (form 5): row 0 of 8 sequences, its target at 8 different key positions; one-hot and two-hot bit for
    bit, peaked and offset within the tolerance AND byte for byte row 0 of attention_rows64 (form 3)"""
    lib, B, H = lab_build, 8, 12
    ok = _allowed(S, 0)
    seed = 7000 + S
    shifts = np.array([0, 1, 15, 16, 17, S - 1, 7, 33])
    t = (np.arange(S)[None, :] + shifts[:, None]) % S                            # [B, S]
    q, k, v = one_hot(seed, B, H, S, t)
    _assert_one_hot(Ref(q, k, v, ok, tolerance=False), t, ("a", S))
    want = np.take_along_axis(v, np.broadcast_to(t[:, None, :, None], v.shape), axis=2)
    assert np.array_equal(_launch(lib, 5, q, k, v, 0), _bits(_rows(want[:, :, :1]))), ("one-hot row 0 is not V[t(0)] bit for bit", S)
    for a, b in ((0, S - 1), (15, 16)):
        if b <= a or b >= S:
            continue
        q, k, v, want = two_hot(seed + 1 + a, B, H, S, a, b)
        _assert_one_hot(Ref(q, k, v, ok, tolerance=False), np.full(S, a), ("b", S, a, b), pair=b)
        assert np.array_equal(_launch(lib, 5, q, k, v, 0), _bits(_rows(want[:, :, None, :]))), ("two-hot row 0", S, a, b)
    for offset in (False, True):
        q, k, v = peaked(seed + 40 + offset, B, H, S, offset)
        r = Ref(q, k, v, ok)
        r.check_condition(("pooled", S, offset))
        got = _launch(lib, 5, q, k, v, 0)
        d = np.abs(_vals(got).astype(np.float64) - _rows(r.ref[:, :, :1]))
        assert (d <= _rows(r.tol[:, :, :1])).all(), (S, offset, float((d / _rows(r.tol[:, :, :1])).max()))
        full = _launch(lib, 3, q, k, v, 0)
        assert np.array_equal(got, full[::S]), ("attn_pooled_rows is not row 0 of attention_rows64", S, offset)


# ---- the skinny kernel ----------------------------------------------------------------------------------------------
def _skinny(lib, B, L, causal, q, k, v, Wo, bias, res):
    """one launch of skinny_attn_out on R = B L rows given as one tile [1, 8, R, 64]; returns out [R, 512] f32"""
    R, D = B * L, 512
    qkv = _pack(q, k, v)
    Wo_bits = _bits(Wo)
    out = np.full((R, D), np.nan, dtype=np.float32)
    rc = lib.ssw_debug_skinny_attn_out_run(B, L, causal, SCALE, _p(qkv), _p(Wo_bits), _p(bias), _p(res), _p(out))
    assert rc == 0, lib.ssw_last_error().decode()
    assert np.isfinite(out).all(), ("NaN / inf / an unwritten row", B, L, causal)
    return out


def _masked_target(B, L, causal):
    """a key query r must not see: the next row of its sequence (causal, even r), else the same position one sequence on;
    itself where nothing is masked"""
    R = B * L
    r = np.arange(R)
    t = (r + L) % R if B > 1 else r.copy()
    if causal:
        has_next = (r + 1) % L != 0
        t = np.where(has_next & ((r % 2 == 0) | (B == 1)), r + 1, t)
    return t


@gpu
@pytest.mark.parametrize("B,L", [(1, 1), (1, 16), (16, 1), (2, 8), (3, 5), (1, 17), (1, 32), (2, 16), (32, 1), (4, 8), (3, 9), (5, 6)])
def test_skinny_attention_outprojection(lab_build, B, L):
    """skinny_attn_out<1> (<= 16 rows) and <2> (17 .. 32): block-causal and block-only masks.  Behind Wo = identity, bias
    = 0, residual = 0 the f32 output IS the attention output: families (a) and (b) bit for bit.  Behind a random Wo
    (std 0.05), bias and residual: (c), (d), (e) within the attention tolerance carried through the product."""
    lib, R, H, D = lab_build, B * L, 8, 512
    seed = 9000 + 100 * B + L
    eye, zero_b, zero_r = np.eye(D, dtype=np.float32), np.zeros(D, np.float32), np.zeros((R, D), np.float32)
    rng = np.random.default_rng(seed)
    Wo = _round(0.05 * rng.standard_normal((D, D)))
    bias = (0.5 * rng.standard_normal(D)).astype(np.float32)
    res = rng.standard_normal((R, D)).astype(np.float32)
    for causal in (0, 1):
        ok = _allowed(R, causal, L)
        for s in SHIFTS:                                                        # (a)
            t = _shift_target(R, s, causal, L)
            q, k, v = one_hot(seed + 10 + s, 1, H, R, t)
            _assert_one_hot(Ref(q, k, v, ok, tolerance=False), t, ("a", B, L, causal, s))
            want = _rows(np.take_along_axis(v, np.broadcast_to(t[None, None, :, None], v.shape), axis=2))
            got = _skinny(lib, B, L, causal, q, k, v, eye, zero_b, zero_r)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("one-hot", B, L, causal, s)
        if not causal:                                                          # (b), inside every sequence
            for a, b in ((0, L - 1), (15, 16)):
                if b <= a or b >= L:
                    continue
                rngb = np.random.default_rng(seed + 20 + a)
                k = _keys(rngb, 1, H, R)
                v = _int_values(rngb, (1, H, R, 64))
                first = np.arange(R) // L * L
                k[:, :, first + b] = k[:, :, first + a]
                v[:, :, first + b] = np.where(v[:, :, first + a] + v[:, :, first + b] == 0, v[:, :, first + a], v[:, :, first + b])
                q = _aimed(k, first + a)
                P = Ref(q, k, v, ok, tolerance=False).P
                w, w2 = (np.take_along_axis(P, np.broadcast_to((first + c)[None, None, :, None], (1, H, R, 1)), axis=3) for c in (a, b))
                assert np.array_equal(w, w2) and (w + w2 >= 1 - 2.0 ** -20).all(), ("two-hot condition missed", B, L, a, b)
                want = _rows(0.5 * (v[:, :, first + a] + v[:, :, first + b]))
                got = _skinny(lib, B, L, causal, q, k, v, eye, zero_b, zero_r)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("two-hot", B, L, a, b)
        cases = [("c", needle(seed + 50 + causal, 1, H, R, _masked_target(B, L, causal))),
                 ("d", peaked(seed + 30 + causal, 1, H, R)), ("e", peaked(seed + 40 + causal, 1, H, R, offset=True))]
        for name, (q, k, v) in cases:
            r = Ref(q, k, v, ok)
            r.check_condition((name, B, L, causal))
            att, tol_att = _rows(r.ref), _rows(r.tol)
            W64 = Wo.astype(np.float64)
            ref = att @ W64.T + bias + res
            tol = tol_att @ np.abs(W64).T + 520 * 2.0 ** -24 * ((np.abs(att) + tol_att) @ np.abs(W64).T + np.abs(bias) + np.abs(res))
            got = _skinny(lib, B, L, causal, q, k, v, Wo, bias, res)
            d = np.abs(got - ref)
            print(f"skinny {name} B={B} L={L} causal={causal}: max |got - ref| / tol = {float((d / tol).max()):.3f}")
            assert (d <= tol).all(), (name, B, L, causal, float((d / tol).max()), float(d.max()))


# ---- refusals -------------------------------------------------------------------------------------------------------
@gpu
def test_refused_shapes_launch_nothing(lab_build):
    """a shape a form cannot hold is SSW_ERR_UNSUPPORTED with a message, the out buffer comes back untouched, and the
    library serves the next call"""
    lib = lab_build
    refused = [(f, 65, 768, 12, 0) for f in (0, 1, 3, 5)] + [(2, 81, 768, 12, 0), (4, 273, 768, 12, 0)]
    refused += [(f, 0, 768, 12, 0) for f in range(6)] + [(f, 16, 768, 8, 0) for f in range(6)] + [(5, 16, 768, 12, 1)]
    for form, S, D, H, causal in refused:
        rows = 3 * max(S, 1) + QKV_GUARD
        qkv = np.full((rows, 3 * D), 0x7FC0, dtype=np.uint16)
        out = _sentinel((rows, D))
        before = out.copy()
        rc = lib.ssw_debug_attention_run(form, 3, S, D, H, causal, SCALE, _p(qkv), rows, _p(out), rows)
        assert rc == -4 and lib.ssw_last_error(), (form, S, D, H, causal, rc)
        assert np.array_equal(out, before), (form, S, D, H, causal)
    z = np.zeros((33, 1536), dtype=np.uint16)
    W, b, res, out = np.zeros((512, 512), np.uint16), np.zeros(512, np.float32), np.zeros((33, 512), np.float32), np.full((33, 512), 7.0, np.float32)
    for B, L in ((33, 1), (1, 33), (3, 11), (0, 4), (4, 0)):
        assert lib.ssw_debug_skinny_attn_out_run(B, L, 1, SCALE, _p(z), _p(W), _p(b), _p(res), _p(out)) == -4
        assert (out == 7.0).all()
    q, k, v = peaked(1, 3, 12, 16)
    r = Ref(q, k, v, _allowed(16, 0))
    _assert_close(_launch(lib, 3, q, k, v, 0), r, "the call behind the refusals")


# ---- the fused image launch -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 63, 64])
def test_fused_image_launch_on_the_same_inputs(lab_build, S):
    """csrc/attn_out.hip through ssw_debug_attn_out_run, f32 rows, Wo = identity, bo = 0, res_in = 0: res_out IS the
    attention output.  (a), (b): the expected rows bit for bit; (d), (e): as bf16 bits, attention_rows64's output byte for
    byte.  xcopy is its rounding, the partial statistics are those of the row as stored (test_gemm_gpu.py's tolerances)."""
    lib, B, H, D = lab_build, 3, 12, 768
    ok = _allowed(S, 0)
    seed = 11000 + S
    Wo = _bits(np.eye(D, dtype=np.float32))
    bo, res_in = np.zeros(D, np.float32), np.zeros((B * S, D), np.float32)

    def fused(q, k, v):
        qkv = _pack(q, k, v)
        xs = _sentinel((B * S, D))
        res_out = np.full((B * S, D), np.nan, dtype=np.float32)
        stats = np.full((B * S, 2, 2), np.nan, dtype=np.float32)
        rc = lib.ssw_debug_attn_out_run(B, S, _p(qkv), _p(Wo), _p(bo), _p(xs), _p(res_in), _p(res_out), _p(stats), SCALE)
        assert rc == 0, lib.ssw_last_error().decode()
        assert np.isfinite(res_out).all() and np.isfinite(stats).all()
        assert np.array_equal(xs, _bits(res_out))
        h = res_out.reshape(B * S, 2, D // 2).astype(np.float64)
        assert np.allclose(stats[:, :, 0], h.sum(2), rtol=0, atol=3e-3) and np.allclose(stats[:, :, 1], (h * h).sum(2), rtol=3e-5, atol=3e-3)
        return res_out

    for s in SHIFTS:
        t = _shift_target(S, s, 0)
        q, k, v = one_hot(seed + 10 + s, B, H, S, t)
        _assert_one_hot(Ref(q, k, v, ok, tolerance=False), t, ("a", S, s))
        want = _rows(np.take_along_axis(v, np.broadcast_to(t[None, None, :, None], v.shape), axis=2))
        assert np.array_equal(fused(q, k, v).view(np.uint32), want.view(np.uint32)), ("one-hot", S, s)
    for a, b in ((0, S - 1), (15, 16)):
        if b <= a or b >= S:
            continue
        q, k, v, want = two_hot(seed + 20 + a, B, H, S, a, b)
        _assert_one_hot(Ref(q, k, v, ok, tolerance=False), np.full(S, a), ("b", S, a, b), pair=b)
        want = _rows(np.broadcast_to(want[:, :, None, :], v.shape))
        assert np.array_equal(fused(q, k, v).view(np.uint32), want.view(np.uint32)), ("two-hot", S, a, b)
    for offset in (False, True):
        q, k, v = peaked(seed + 40 + offset, B, H, S, offset)
        r = Ref(q, k, v, ok)
        r.check_condition(("fused", S, offset))
        res_out = fused(q, k, v)
        rows64 = _launch(lib, 3, q, k, v, 0)
        assert np.array_equal(_vals(rows64), res_out), ("the fused launch's rows are not attention_rows64's", S, offset)
        _assert_close(rows64, r, f"fused S={S} offset={offset}")


# ---- the inputs and the tolerance themselves, on the CPU ------------------------------------------------------------
def _emulate(q, k, v, allowed):
    """the kernels' rounding sequence in numpy: f32 logits, f32 exp of (logit - max), normalised in f32, P to bf16, f32
    product, output to bf16"""
    f = np.float32
    logits = (q.astype(f) @ k.astype(f).transpose(0, 1, 3, 2)) * f(SCALE)
    logits = np.where(allowed, logits, f(-np.inf))
    e = np.exp(logits - logits.max(axis=-1, keepdims=True), dtype=f)
    p = _round(e * (f(1) / e.sum(axis=-1, keepdims=True, dtype=f)))
    return _round(p @ v.astype(f))


def test_peaked_inputs_and_tolerance_on_the_cpu():
    """no GPU: the statistics the docstring quotes for family (d), the one-hot condition at the longest length, the
    'f32 term <= half the bf16 term' condition, and a numpy emulation of the rounding sequence inside the tolerance --
    and bit-exact on the one-hot and two-hot families"""
    B, H = 3, 12
    for S in (17, 64, 80, 197, 272):
        for causal in (0, 1):
            ok = _allowed(S, causal)
            for offset in (False, True):
                q, k, v = peaked(100 + S + causal, B, H, S, offset)
                r = Ref(q, k, v, ok)
                r.check_condition((S, causal, offset))
                d = np.abs(_emulate(q, k, v, ok).astype(np.float64) - r.ref)
                assert (d <= r.tol).all(), (S, causal, offset, float((d / r.tol).max()))
                if not causal and not offset:
                    logits = SCALE * (q.astype(np.float64) @ k.astype(np.float64).transpose(0, 1, 3, 2))
                    assert 3.7 <= logits.std() <= 4.3, logits.std()
                    assert 0.45 <= np.median(r.P.max(axis=-1)) <= 0.8, (S, float(np.median(r.P.max(axis=-1))))
            t = _shift_target(S, 17, causal)
            q, k, v = one_hot(S, B, H, S, t)
            _assert_one_hot(Ref(q, k, v, ok, tolerance=False), t, (S, causal))
            want = np.take_along_axis(v, np.broadcast_to(t[None, None, :, None], v.shape), axis=2)
            assert np.array_equal(_emulate(q, k, v, ok), want)
        q, k, v, want = two_hot(S, B, H, S, 0, S - 1)
        assert (want != 0).all()
        assert np.array_equal(_emulate(q, k, v, _allowed(S, 0)), np.broadcast_to(want[:, :, None, :], v.shape))
    keys = _sign_keys()
    g = keys @ keys.T
    assert (g[~np.eye(272, dtype=bool)] <= 32).all() and (np.diag(g) == 64).all()
