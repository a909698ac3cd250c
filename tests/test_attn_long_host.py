"""Argument validation of the long-caption attention entry points (glr_attn_long_fwd / _bwd, include/glr.h) without a
device: every bad argument is refused with GLR_EINVAL before any HIP call, so none of these calls touches a GPU (the
pointers are made-up non-NULL addresses that nothing may dereference).  The short kernels' bound stays 128."""

EINVAL = -1            # include/glr.h
FAKE = 0x10000         # a non-NULL address: the calls below must return before using it


def test_long_max_tokens():
    from gloria import _native as N
    assert N.lib().glr_attn_long_max_tokens() == 512


def test_short_max_tokens_unchanged():
    from gloria import _native as N
    Lb = N.lib()
    assert Lb.glr_attn_max_tokens(0) == Lb.glr_attn_max_tokens(1) == 128


def test_long_entry_points_refuse_bad_arguments_before_a_launch():
    from gloria import _native as N
    Lb = N.lib()
    B, nh = 1, 2
    H = 64 * nh

    def fwd(L=258, ld=H, ld_o=H, p=0.1, keep=FAKE, o=FAKE, lse=FAKE):
        return Lb.glr_attn_long_fwd(FAKE, FAKE, FAKE, FAKE, B, nh, L, ld, ld_o, 0.125, p, 1, 0, None, o, lse, keep, None)

    def bwd(L=258, ld=H, ld_o=H, p=0.1, keep=FAKE, o=FAKE, lse=FAKE, dq=FAKE):
        return Lb.glr_attn_long_bwd(FAKE, FAKE, FAKE, o, FAKE, FAKE, lse, keep, B, nh, L, ld, ld_o, 0.125, p, dq, FAKE, FAKE, None)

    bad = [dict(L=0), dict(L=513), dict(L=-3), dict(ld=H - 8), dict(ld=H + 4), dict(ld_o=H - 8), dict(ld_o=H + 4), dict(p=1.0),
           dict(p=-0.1), dict(keep=None), dict(o=None), dict(lse=None)]
    for kw in bad:
        assert fwd(**kw) == EINVAL, ("fwd", kw)
        assert bwd(**kw) == EINVAL, ("bwd", kw)
    assert bwd(dq=None) == EINVAL
    # NULL q / k / v and empty batches
    assert Lb.glr_attn_long_fwd(None, FAKE, FAKE, None, B, nh, 258, H, H, 0.125, 0.0, 1, 0, None, FAKE, FAKE, None, None) == EINVAL
    assert Lb.glr_attn_long_fwd(FAKE, FAKE, FAKE, None, 0, nh, 258, H, H, 0.125, 0.0, 1, 0, None, FAKE, FAKE, None, None) == EINVAL
    assert Lb.glr_attn_long_fwd(FAKE, FAKE, FAKE, None, B, 0, 258, H, H, 0.125, 0.0, 1, 0, None, FAKE, FAKE, None, None) == EINVAL
    # the short entry points still refuse 129 tokens
    assert Lb.glr_attn_fwd(FAKE, FAKE, FAKE, None, B, nh, 129, H, H, 0.125, 0.0, 1, 0, None, FAKE, FAKE, None, None) == EINVAL
