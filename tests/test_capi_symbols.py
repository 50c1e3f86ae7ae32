"""The C-ABI library builds, loads without a GPU, and exports every symbol that
include/scl_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_surface():
    names = _declared()
    for want in ("scl_netvlad_fwd", "scl_netvlad_bwd", "scl_gram_loss_fwd", "scl_gram_loss_bwd",
                 "scl_tuple_loss_fwd", "scl_tuple_loss_bwd", "scl_logratio_fwd",
                 "scl_pairwise_sqdist", "scl_topn_l2", "scl_abi_version", "scl_error_string"):
        assert want in names


def test_every_declared_symbol_is_exported_and_bound(lib):
    from soft_contrastive_learning_amd import _lib
    declared = _declared()
    assert sorted(_lib.SIGNATURES) == declared
    for name in declared:
        assert getattr(lib, name) is not None


def test_product_library_has_no_variants_and_the_diagnostic_build_does(lib):
    """csrc/Makefile builds the sources twice: libscl_hip.so (what load() returns) is compiled
    without -DSCL_DIAG — scl_variant() is the constant 0 there, no variant branch survives — and
    refuses every selector but 0; libscl_hip_diag.so exports the same surface with the switch."""
    from soft_contrastive_learning_amd import _lib
    assert lib.scl_build_is_diag() == 0
    assert lib.scl_debug_set_variant(0) == 0
    assert lib.scl_debug_set_variant(921) == -2 and lib.scl_debug_set_variant(0) == 0
    diag = _lib.load(diag=True)
    assert diag is not lib and diag.scl_build_is_diag() == 1
    for name in _declared():
        assert getattr(diag, name) is not None
    assert diag.scl_debug_set_variant(921) == 0 and diag.scl_debug_set_variant(0) == 921
    with _lib.variant(32) as inside:
        assert inside is diag and _lib.load() is diag
    assert _lib.load() is lib and diag.scl_debug_set_variant(0) == 0
    # the product object files carry no reference to the switch at all
    import subprocess
    so = os.path.join(ROOT, 'soft_contrastive_learning_amd', 'libscl_hip.so')
    syms = subprocess.run(['nm', '-D', so], capture_output=True, text=True).stdout
    assert 'scl_debug_variant' not in syms.replace('scl_debug_set_variant', '')
    syms = subprocess.run(['nm', '-D', so.replace('.so', '_diag.so')], capture_output=True, text=True).stdout
    assert 'scl_debug_variant' in syms.replace('scl_debug_set_variant', '')
    # nor any kernel that only a variant launches: those live in csrc/*_diag.hip, which the
    # diagnostic library alone compiles (the device code is stored uncompressed in both)
    product, diagnostic = open(so, 'rb').read(), open(so.replace('.so', '_diag.so'), 'rb').read()
    for name in (b'rowtile16_kernelIfLi0ELi1E', b'rowtile16_kernelItLi0ELi7E', b'wrw64_kernelILi2E',
                 b'wrw64_kernelILi4E', b'wrw64_kernelILi6E', b'wrw64_kernelILi8E', b'wrw64_kernelILi16E',
                 b'vlad_split_w_kernel', b'vlad_fwd_kernelILb1E', b'vlad_bwd_kernel', b'vlad_finish_sum_kernel',
                 b'vlad_wgrad_partial_kernel', b'bwd_dots_kernel', b'bwd_du_kernel', b'persist_kernel',
                 b'gram16x6_kernelILi9ELi2ELb1E', b'gram16x6_kernelILi20ELi2ELb1E',
                 b'conv3x3_kernelILi64ELi64ELi0ELi0ELi0ELi1E',
                 b'convh_kernelILi0ELi12E', b'convh_kernelILi1ELi12E', b'convh_kernelILi2ELi12E',
                 b'convh_kernelILi3ELi12E', b'convh_kernelILi1ELi24ELb1E'):
        assert name not in product, name
        assert name in diagnostic, name
    # ... and every LDS-weights kernel the product launchers (csrc/convh.hip, csrc/convg.hip) can choose
    kept = ['convh_kernelILi%dELi%dELb0ELb%dE' % (e, bh, full) for e in range(4) for bh in (24, 8, 6)
            for full in (0, 1)] + ['convg_kernelILi%dELi%dE' % (e, bh) for e in range(4) for bh in (12, 8)]
    for name in kept:
        assert name.encode() in product, name
        assert name.encode() in diagnostic, name


def test_abi_version_and_error_strings(lib):
    assert lib.scl_abi_version() == 12
    assert lib.scl_error_string(0) == b"ok"
    assert b"shape" in lib.scl_error_string(-1)
    assert b"NULL" in lib.scl_error_string(-3)


def test_workspace_queries_are_pure_host_functions(lib):
    # NetVLAD forward at the bench shape: Wt + slabs + a + rn, all 256-byte rounded
    n = lib.scl_netvlad_fwd_workspace_bytes(24, 1200)
    assert n >= 24 * 2 * 512 * 64 * 4 + 24 * 1200 * 64 * 4
    assert n % 256 == 0
    assert lib.scl_netvlad_fwd_workspace_bytes(0, 10) == 0
    assert lib.scl_netvlad_bwd_workspace_bytes(24, 1200) % 256 == 0
    assert lib.scl_gram_loss_workspace_bytes(24, 32768) > 0
    assert lib.scl_gram_loss_workspace_bytes(5000, 32768) == 0          # B above the cap
    # both sides of every route boundary of the forward (fused | float32 Gram | strip-scheduled bf16x6 |
    # bf16x6 | 32x32 tiles), E a multiple of the bf16x6 slice and not: the byte counts of the library
    # before the forward's routes and this query read one plan
    want = {
        (32, 128): 22016, (32, 200): 28160, (32, 32768): 212480,
        (33, 128): 32768, (33, 200): 45056, (33, 32768): 1593344,
        (64, 128): 80384, (64, 200): 100864, (64, 32768): 2681344,
        (65, 128): 98560, (65, 200): 129280, (65, 32768): 4000000,
        (208, 128): 800768, (208, 200): 987136, (208, 32768): 24469504,
        (209, 128): 849152, (209, 200): 1064192, (209, 32768): 28159232,
        (256, 128): 1206272, (256, 200): 1484800, (256, 32768): 36579328,
        (257, 128): 1689856, (257, 200): 2242816, (257, 32768): 5007616,
    }
    got = {k: lib.scl_gram_loss_workspace_bytes(*k) for k in want}
    assert got == want
    assert lib.scl_topn_l2_workspace_bytes(100000, 10000, 256, 25) > 100000 * 4
    assert lib.scl_topn_l2_workspace_bytes(100, 10, 100, 5) == 0         # unsupported d
    assert lib.scl_topn_l2_workspace_bytes(100, 10, 64, 26) == 0         # n above the cap


def test_argument_validation_happens_before_any_launch(lib):
    # NULL pointers and bad selectors are rejected on the host: safe without a GPU
    assert lib.scl_gram_loss_fwd(None, 0, 4, 8, 0, None, 0, 0.8, 15.0, None, 2.0, 50.0, 1.0, 0.1,
                                 1, 0, None, None, None, 0, None) == -3
    assert lib.scl_tuple_loss_fwd(99, None, 0, None, 0, None, 0, None, 0, 1, 1, 1, 8, 0.1, 0.2,
                                  None, None, None, None) == -2
    assert lib.scl_netvlad_fwd(None, 0, None, None, 1, 1, 1, None, None, None, None, None, None, 0,
                               None) == -3
    assert lib.scl_topn_l2(None, 1, None, 1, 64, 1, 0, None, None, None, 0, None) == -3


def test_pooled_backward_entry_points_validate_on_the_host(lib):
    """scl_wrw3x3_pooled / scl_conv3x3_masked_pooled (round 3): NULL operands, odd map sizes and
    shapes the un-pooling staging does not exist for are refused before any launch."""
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws_bytes = lib.scl_wrw3x3_workspace_bytes(64, 64)
    assert ws_bytes > 0 and lib.scl_wrw3x3_workspace_bytes(48, 64) == 0
    # NULL index / NULL gradient
    assert lib.scl_wrw3x3_pooled(p, p, None, 1, 8, 8, 64, 64, p, 576, 9, 3, 1, 1, None, p, ws_bytes,
                                 None) == -3
    assert lib.scl_wrw3x3_pooled(p, None, p, 1, 8, 8, 64, 64, p, 576, 9, 3, 1, 1, None, p, ws_bytes,
                                 None) == -3
    # channel counts without a kernel (-1 = shape), odd height (a 2x2 window would straddle the edge)
    assert lib.scl_wrw3x3_pooled(p, p, p, 1, 8, 8, 48, 64, p, 432, 9, 3, 1, 1, None, p, 1 << 20,
                                 None) == -1
    assert lib.scl_wrw3x3_pooled(p, p, p, 1, 7, 8, 64, 64, p, 576, 9, 3, 1, 1, None, p, ws_bytes,
                                 None) == -1
    cw = lib.scl_conv3x3_workspace_bytes()
    assert lib.scl_conv3x3_masked_pooled(p, None, p, 576, 9, 3, 1, 1, 1, 8, 8, 64, 64, p, p, p, cw,
                                         None) == -3
    assert lib.scl_conv3x3_masked_pooled(p, p, p, 576, 9, 3, 1, 1, 1, 8, 8, 64, 64, p, None, p, cw,
                                         None) == -3
    # cin != kout has no un-pooling window staging; odd width
    assert lib.scl_conv3x3_masked_pooled(p, p, p, 576, 9, 3, 1, 1, 1, 8, 8, 128, 64, p, p, p, cw,
                                         None) == -1
    assert lib.scl_conv3x3_masked_pooled(p, p, p, 576, 9, 3, 1, 1, 1, 8, 9, 64, 64, p, p, p, cw,
                                         None) == -1


def test_lds_convolution_entry_points_validate_on_the_host(lib):
    """scl_convg / scl_convg_masked / scl_convg_pool_idx (csrc/conv_lds.hip): every refusal of the
    argument checks, in their order of precedence, comes back before any launch.  (Two of the
    checks — an index map with a mask, a mask with a bias — guard combinations no entry point forms.)"""
    from soft_contrastive_learning_amd import _lib
    NULL, SHAPE, WORKSPACE, KIND = -3, -1, -4, -2
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)       # 256-byte / only 8-byte aligned
    ws = lib.scl_convg_workspace_bytes(160, 128)
    assert ws > 0 and ws % 256 == 0 and lib.scl_convg_workspace_bytes(48, 128) == 0
    assert lib.scl_convg_workspace_bytes(128, 64) == 0 and lib.scl_convg_workspace_bytes(2048, 128) == 0

    def conv(x=p, w=p, flags=0, b=1, h=8, wd=8, cin=160, kout=128, out=p, work=p, nbytes=ws):
        return lib.scl_convg(x, w, 1, 1, 1, 1, flags, b, h, wd, cin, kout, out, None, 0, work, nbytes, None)

    def masked(mask=p, cin=160, nbytes=ws):
        return lib.scl_convg_masked(p, p, 1, 1, 1, 1, 0, 1, 8, 8, cin, 128, p, mask, p, nbytes, None)

    def pool(bias=p, pooled=p, idx=p, cin=160, flags=0, nbytes=ws):
        return lib.scl_convg_pool_idx(p, p, 1, 1, 1, 1, flags, 1, 8, 8, cin, 128, bias, pooled, idx, p, nbytes, None)

    # NULL operands — before the shape: cin = 48 has no kernel
    for kw in (dict(x=None), dict(w=None), dict(out=None), dict(work=None)):
        assert conv(cin=48, **kw) == NULL, kw
    assert masked(mask=None) == NULL and masked(mask=odd, cin=48) == NULL     # mask NULL / not 16-byte aligned
    assert pool(bias=None) == NULL and pool(pooled=None) == NULL and pool(idx=None, cin=48) == NULL
    # shapes — before the workspace
    assert conv(cin=48) == SHAPE and conv(kout=64) == SHAPE and conv(cin=2048) == SHAPE
    assert conv(b=0) == SHAPE and conv(h=0) == SHAPE and conv(wd=0) == SHAPE
    assert conv(b=1 << 11, h=1 << 10, wd=1 << 10) == SHAPE                   # more than 2^30 pixels
    assert conv(x=odd) == SHAPE and conv(out=odd, nbytes=0) == SHAPE         # not 16-byte aligned
    assert conv(b=1 << 10, h=1 << 7, wd=1 << 7, cin=128) == SHAPE            # B H W cin = 2^31
    assert masked(cin=48) == SHAPE and pool(cin=48) == SHAPE
    # workspace: too small, not 256-byte aligned — before the weight format
    assert conv(nbytes=ws - 1) == WORKSPACE and conv(work=odd) == WORKSPACE
    assert masked(nbytes=ws - 1) == WORKSPACE and pool(nbytes=ws - 1) == WORKSPACE
    assert conv(flags=_lib.W_PACKED, nbytes=0) == WORKSPACE
    # packed images exist in the 16x16x32 kernel's layout only, and five 32-channel chunks go to the other
    assert conv(flags=_lib.W_PACKED) == KIND and pool(flags=_lib.W_PACKED) == KIND
    # ... so a packed image is refused too where the diagnostic build pins the other kernel (40000 + v)
    ws2 = lib.scl_convg_workspace_bytes(256, 128)
    big = ctypes.create_string_buffer(ws2 + 256)
    q = ctypes.c_void_p((ctypes.addressof(big) + 255) & ~255)
    with _lib.variant(40000) as diag:
        assert diag.scl_convg(q, q, 1, 1, 1, 1, _lib.W_PACKED, 1, 8, 8, 256, 128, q, None, 0, q, ws2, None) == KIND


def test_register_convolution_entry_points_validate_on_the_host(lib):
    """The register-weights family of csrc/conv64.hip — scl_conv3x3_fused / _pool_idx / _masked /
    _masked_pooled (and the legacy scl_conv3x3, scl_conv64) — the weight gradient of csrc/conv_wrw.hip —
    scl_wrw3x3_bias / _pooled (and scl_wrw3x3_ex, scl_wrw3x3, scl_wrw64) — and the first-layer entry points: every
    refusal comes back before any launch, each asserted with a condition that a LATER check refuses
    also present, so the order of precedence is pinned.  (Three of the convolution's checks — an
    index map with a mask, a mask with a bias, an un-pooling index without a mask — guard combinations
    no entry point forms: scl_conv3x3_masked_pooled refuses a NULL mask itself, with NULL.)"""
    NULL, SHAPE, WORKSPACE = -3, -1, -4
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p = ctypes.c_void_p(base)
    a16, a8, a4 = ctypes.c_void_p(base + 16), ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 4)
    cw = lib.scl_conv3x3_workspace_bytes()

    # ---- the convolution: checks 1 .. 10 of the front door, in its order -------------------------
    def fused(x=p, w=p, b=1, h=8, wd=8, cin=64, kout=64, out=p, bias=None, pooled=None, work=p, nbytes=cw):
        return lib.scl_conv3x3_fused(x, w, 1, 1, 1, 1, 0, b, h, wd, cin, kout, out, bias, 0, pooled, work,
                                     nbytes, None)

    def pool(bias=p, pooled=p, idx=p, b=1, cin=64, nbytes=cw):
        return lib.scl_conv3x3_pool_idx(p, p, 1, 1, 1, 1, 0, b, 8, 8, cin, 64, bias, pooled, idx, p, nbytes, None)

    def masked(mask=p, b=1, cin=64, nbytes=cw):
        return lib.scl_conv3x3_masked(p, p, 1, 1, 1, 1, 1, b, 8, 8, cin, 64, p, mask, p, nbytes, None)

    def unpool(idx=p, mask=p, h=8, wd=8, cin=64, kout=64, b=1, nbytes=cw):
        return lib.scl_conv3x3_masked_pooled(p, idx, p, 1, 1, 1, 1, 1, b, h, wd, cin, kout, p, mask, p, nbytes,
                                             None)

    # 1: NULL x / w / workspace, out with no index map — before the shape (cin = 48 has no kernel)
    for kw in (dict(x=None), dict(w=None), dict(work=None), dict(out=None)):
        assert fused(cin=48, nbytes=0, **kw) == NULL, kw
    assert pool(idx=None, cin=48) == NULL and pool(pooled=None, b=0) == NULL and pool(bias=None, b=0) == NULL
    assert masked(mask=None, b=0) == NULL
    assert unpool(mask=None, h=7) == NULL and unpool(idx=None, h=7) == NULL
    # 2: the un-pooling window staging (cin == kout, even H and W, index 8-byte aligned): SHAPE — before
    # the NULL of a mask that is not 16-byte aligned (4)
    assert unpool(cin=128, kout=64, mask=a8) == SHAPE and unpool(cin=64, kout=128, mask=a8) == SHAPE
    assert unpool(h=7, mask=a8) == SHAPE and unpool(wd=9, mask=a8) == SHAPE
    assert unpool(idx=a4, mask=a8) == SHAPE
    assert unpool(mask=a8, b=0) == NULL                              # ... which then comes before 7
    # 3: an index map that is not 8-byte aligned: NULL — before the shape (7)
    assert pool(idx=a4, b=0) == NULL
    # 4: a mask that is not 16-byte aligned: NULL, not SHAPE — before the shape (7)
    assert masked(mask=a8, b=0) == NULL and masked(mask=a8, cin=48) == NULL
    # 5: B H W cin = 2^31: SHAPE — before the NULL of a pooled output without its bias (6)
    assert fused(b=1 << 10, h=1 << 7, wd=1 << 8, pooled=p) == SHAPE
    assert fused(b=1 << 10, h=1 << 7, wd=1 << 7, cin=128, kout=128, pooled=a8, bias=p) == SHAPE
    # 6: pooled without the bias, pooled not 16-byte aligned: NULL — before the shape (7)
    assert fused(pooled=p, b=0) == NULL and fused(pooled=a8, bias=p, b=0) == NULL
    assert pool(pooled=a8, b=0) == NULL
    # 7: empty maps, more than 2^30 pixels: SHAPE — before the workspace (9)
    assert fused(b=0, nbytes=0) == SHAPE and fused(h=0, nbytes=0) == SHAPE and fused(wd=0, nbytes=0) == SHAPE
    assert fused(b=1 << 11, h=1 << 10, wd=1 << 10, nbytes=0) == SHAPE
    assert pool(b=0, nbytes=0) == SHAPE and masked(b=0, nbytes=0) == SHAPE and unpool(b=0, nbytes=0) == SHAPE
    # 8: x or out not 16-byte aligned: SHAPE — before the workspace (9)
    assert fused(x=a8, nbytes=0) == SHAPE and fused(out=a8, nbytes=0) == SHAPE
    assert fused(x=a8, work=a16) == SHAPE
    # 9: a workspace one byte short, or not 256-byte aligned: WORKSPACE — before the channel counts (10)
    assert fused(nbytes=cw - 1, kout=96) == WORKSPACE and fused(work=a16, kout=96) == WORKSPACE
    assert pool(nbytes=cw - 1, cin=48) == WORKSPACE and masked(nbytes=cw - 1, cin=48) == WORKSPACE
    assert unpool(nbytes=cw - 1, cin=192, kout=192) == WORKSPACE
    # 10: channel counts without a register kernel
    assert fused(kout=96) == SHAPE and fused(cin=48) == SHAPE and fused(cin=256, kout=256) == SHAPE
    assert pool(cin=48) == SHAPE and masked(cin=48) == SHAPE and unpool(cin=192, kout=192) == SHAPE
    # the legacy names reach the same checks
    assert lib.scl_conv3x3(None, p, 1, 1, 1, 1, 0, 1, 8, 8, 48, 64, p, p, 0, None) == NULL
    assert lib.scl_conv3x3(p, p, 1, 1, 1, 1, 0, 1, 8, 8, 64, 64, None, p, cw, None) == NULL
    assert lib.scl_conv3x3(p, p, 1, 1, 1, 1, 0, 0, 8, 8, 64, 64, p, p, 0, None) == SHAPE
    assert lib.scl_conv3x3(p, p, 1, 1, 1, 1, 0, 1, 8, 8, 64, 96, p, p, cw - 1, None) == WORKSPACE
    assert lib.scl_conv3x3(p, p, 1, 1, 1, 1, 0, 1, 8, 8, 64, 96, p, p, cw, None) == SHAPE
    assert lib.scl_conv64(p, None, 1, 1, 1, 1, 0, 0, 8, 8, p, p, 0, None) == NULL
    assert lib.scl_conv64(p, p, 1, 1, 1, 1, 0, 1, 0, 8, p, p, 0, None) == SHAPE
    assert lib.scl_conv64(a8, p, 1, 1, 1, 1, 0, 1, 8, 8, p, p, 0, None) == SHAPE
    assert lib.scl_conv64(p, p, 1, 1, 1, 1, 0, 1, 8, 8, p, p, cw - 1, None) == WORKSPACE

    # ---- the weight gradient ---------------------------------------------------------------------
    ww = lib.scl_wrw3x3_workspace_bytes(64, 64)

    def wrw(x=p, gz=p, gw=p, b=1, h=8, wd=8, cin=64, kout=64, work=p, nbytes=ww):
        return lib.scl_wrw3x3_bias(x, gz, b, h, wd, cin, kout, gw, 1, 1, 1, 1, 0, None, work, nbytes, None)

    def wrw_pooled(idx=p, gz=p, h=8, wd=8, cin=64, b=1, nbytes=ww):
        return lib.scl_wrw3x3_pooled(p, gz, idx, b, h, wd, cin, 64, p, 1, 1, 1, 1, 0, None, p, nbytes, None)

    for kw in (dict(x=None), dict(gz=None), dict(gw=None), dict(work=None)):
        assert wrw(cin=48, nbytes=0, **kw) == NULL, kw
    assert wrw_pooled(idx=None, cin=48) == NULL and wrw_pooled(gz=None, h=7) == NULL
    # an index map: odd H or W, or not 8-byte aligned — SHAPE before the workspace
    assert wrw_pooled(h=7, nbytes=0) == SHAPE and wrw_pooled(wd=9, nbytes=0) == SHAPE
    assert wrw_pooled(idx=a4, nbytes=0) == SHAPE
    assert wrw(cin=48, nbytes=0) == SHAPE and wrw(kout=1088, nbytes=0) == SHAPE and wrw_pooled(cin=48, nbytes=0) == SHAPE
    assert wrw(b=0, nbytes=0) == SHAPE and wrw(h=0, nbytes=0) == SHAPE and wrw(wd=0, nbytes=0) == SHAPE
    assert wrw(b=1 << 11, h=1 << 10, wd=1 << 10, nbytes=0) == SHAPE          # more than 2^30 pixels
    assert wrw(b=1 << 10, h=1 << 7, wd=1 << 7, cin=64, kout=128, nbytes=0) == SHAPE   # B H W max(cin, kout) = 2^31
    assert wrw(x=a8, nbytes=0) == SHAPE and wrw(gz=a8, nbytes=0) == SHAPE    # not 16-byte aligned
    assert wrw(nbytes=ww - 1) == WORKSPACE and wrw(work=a16) == WORKSPACE and wrw_pooled(nbytes=ww - 1) == WORKSPACE
    assert lib.scl_wrw3x3_ex(p, None, 1, 8, 8, 48, 64, p, 1, 1, 1, 1, 0, p, 0, None) == NULL
    assert lib.scl_wrw3x3_ex(p, p, 1, 8, 8, 48, 64, p, 1, 1, 1, 1, 0, p, 0, None) == SHAPE
    assert lib.scl_wrw3x3_ex(p, p, 1, 8, 8, 64, 64, p, 1, 1, 1, 1, 0, p, ww - 1, None) == WORKSPACE
    assert lib.scl_wrw3x3(p, p, 1, 8, 8, 64, 64, None, 1, 1, 1, 1, p, 0, None) == NULL
    assert lib.scl_wrw3x3(p, p, 0, 8, 8, 64, 64, p, 1, 1, 1, 1, p, 0, None) == SHAPE
    assert lib.scl_wrw3x3(p, p, 1, 8, 8, 64, 64, p, 1, 1, 1, 1, a16, ww, None) == WORKSPACE
    assert lib.scl_wrw64(None, p, 0, 8, 8, p, 1, 1, 1, 1, p, 0, None) == NULL
    assert lib.scl_wrw64(p, p, 0, 8, 8, p, 1, 1, 1, 1, p, 0, None) == SHAPE
    assert lib.scl_wrw64(p, p, 1, 8, 8, p, 1, 1, 1, 1, p, ww - 1, None) == WORKSPACE

    # ---- the first layer -------------------------------------------------------------------------
    def first(img=p, avg=p, w=p, bias=p, x0=p, y=p, b=1, h=8, wd=8):
        return lib.scl_conv_first(img, avg, w, 1, 1, 1, 1, 0, bias, b, h, wd, x0, y, None)

    for kw in (dict(img=None), dict(avg=None), dict(w=None), dict(bias=None), dict(x0=None), dict(y=None)):
        assert first(b=0, **kw) == NULL, kw
    assert first(b=0) == SHAPE and first(h=0) == SHAPE and first(wd=0) == SHAPE
    assert first(b=1 << 11, h=1 << 10, wd=1 << 10) == SHAPE and first(y=a8) == SHAPE

    def first2(b=1, h=8, wd=8, flags=0, work=p, nbytes=cw, **kw):
        a = dict(img=p, avg=p, w1=p, bias1=p, w2=p, bias2=p, x0=p, y1=p, pooled=p, idx=p)
        a.update(kw)
        return lib.scl_conv_first_pool_idx(a['img'], a['avg'], a['w1'], 1, 1, 1, 1, 0, a['bias1'], a['w2'], 1, 1, 1,
                                           1, flags, a['bias2'], b, h, wd, a['x0'], a['y1'], a['pooled'], a['idx'],
                                           work, nbytes, None)

    for name in ('img', 'avg', 'w1', 'bias1', 'w2', 'bias2', 'x0', 'y1', 'pooled', 'idx'):
        assert first2(b=0, **{name: None}) == NULL, name
    assert first2(work=None, b=0) == NULL
    assert first2(b=0, nbytes=0) == SHAPE and first2(h=0, nbytes=0) == SHAPE and first2(wd=0, nbytes=0) == SHAPE
    assert first2(b=1 << 10, h=1 << 7, wd=1 << 8, nbytes=0) == SHAPE                  # B H W 64 = 2^31
    assert first2(y1=a8, nbytes=0) == SHAPE and first2(pooled=a8, nbytes=0) == SHAPE and first2(idx=a4, nbytes=0) == SHAPE
    assert first2(flags=1, nbytes=0) == SHAPE                                         # a transposed conv1_2
    assert first2(nbytes=cw - 1) == WORKSPACE and first2(work=a16) == WORKSPACE

    fw = lib.scl_conv_first_wrw_workspace_bytes()

    def first_wrw(x0=p, gz=p, gw=p, gb=p, w=p, davg=None, b=1, h=8, wd=8, work=p, nbytes=fw):
        return lib.scl_conv_first_wrw(x0, gz, b, h, wd, gw, 1, 1, 1, 1, 0, gb, w, davg, work, nbytes, None)

    for kw in (dict(x0=None), dict(gz=None), dict(gw=None), dict(gb=None), dict(work=None), dict(davg=p, w=None)):
        assert first_wrw(b=0, **kw) == NULL, kw
    assert first_wrw(b=0, nbytes=0) == SHAPE and first_wrw(h=0, nbytes=0) == SHAPE and first_wrw(wd=0, nbytes=0) == SHAPE
    assert first_wrw(b=1 << 10, h=1 << 7, wd=1 << 8, nbytes=0) == SHAPE
    assert first_wrw(gz=a8, nbytes=0) == SHAPE
    assert first_wrw(nbytes=fw - 1) == WORKSPACE and first_wrw(work=a16) == WORKSPACE

    def fused_first(b=1, h=8, wd=8, work=p, nbytes=cw, fwork=p, fbytes=fw, davg=None, **kw):
        a = dict(ga=p, idx=p, w2=p, mask=p, x0=p, gw1=p, gb1=p, w1=p)
        a.update(kw)
        return lib.scl_conv3x3_masked_pooled_first_wrw(
            a['ga'], a['idx'], a['w2'], 1, 1, 1, 1, 0, b, h, wd, a['mask'], a['x0'], a['gw1'], 1, 1, 1, 1, 0,
            a['gb1'], a['w1'], davg, work, nbytes, fwork, fbytes, None)

    for name in ('ga', 'idx', 'w2', 'mask', 'x0', 'gw1', 'gb1'):
        assert fused_first(b=0, **{name: None}) == NULL, name
    assert fused_first(work=None, b=0) == NULL and fused_first(fwork=None, b=0) == NULL
    assert fused_first(davg=p, w1=None, b=0) == NULL
    assert fused_first(b=0, nbytes=0) == SHAPE and fused_first(b=8193, nbytes=0) == SHAPE
    assert fused_first(h=0, nbytes=0) == SHAPE and fused_first(wd=0, nbytes=0) == SHAPE
    assert fused_first(h=7, nbytes=0) == SHAPE and fused_first(wd=9, nbytes=0) == SHAPE
    assert fused_first(b=1 << 10, h=1 << 7, wd=1 << 8, nbytes=0) == SHAPE
    assert fused_first(ga=a8, nbytes=0) == SHAPE and fused_first(mask=a8, nbytes=0) == SHAPE
    assert fused_first(idx=a4, nbytes=0) == SHAPE
    assert fused_first(nbytes=cw - 1) == WORKSPACE and fused_first(work=a16) == WORKSPACE
    assert fused_first(fbytes=fw - 1) == WORKSPACE and fused_first(fwork=a16) == WORKSPACE
    assert fused_first(nbytes=cw - 1, fbytes=0) == WORKSPACE

    # ---- the size queries ------------------------------------------------------------------------
    assert cw == 294912 and fw == 16778240
    want = {(64, 64): 302514688, (64, 128): 302515200, (128, 64): 302252544, (128, 128): 302253056,
            (256, 256): 302123008, (512, 512): 302059520, (1024, 1024): 302030848, (48, 64): 0, (64, 1088): 0}
    assert {k: lib.scl_wrw3x3_workspace_bytes(*k) for k in want} == want
    assert lib.scl_conv64_workspace_bytes() == cw and lib.scl_wrw64_workspace_bytes() == want[(64, 64)]
