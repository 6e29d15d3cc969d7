"""K8 spectrum at every size on the GPU (nae_spectrum_block_ex_f32, the streaming handle, the host node): bit-exact against the
CPU restatement of the canonical FFT (tests/spec_sizes/ref_spectrum.c), and the same bits as the 1024-point kernels at 1024 / 256."""
import ctypes as C

import numpy as np
import pytest

import node_harness
import orc
from test_spectrum_sizes_cpu import SIZES, _build_ref, ref_spectrum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return _build_ref(str(tmp_path_factory.mktemp("ref_spectrum_gpu")))


def bins(n_fft):
    return n_fft // 2 + 1


def gpu_ex(ctx, nae, n_fft, hop, x, ch, n_streams=1, planar=False):
    """x: [n_streams][T*ch] interleaved host samples -> [n_streams, F, ch, bins]"""
    x = np.ascontiguousarray(x, np.float32).reshape(n_streams, -1)
    T = x.shape[1] // ch
    F = ctx.spectrum_frames_ex(T, n_fft, hop)
    B = bins(n_fft)
    host = x if not planar else np.stack([x[s].reshape(T, ch).T.reshape(-1) for s in range(n_streams)])
    d_x, d_o = ctx.array(host), ctx.empty(max(1, n_streams * F * ch * B))
    sig = nae.Sig.planar(d_x.ptr, T, ch) if planar else nae.Sig.interleaved(d_x.ptr, T, ch)
    ctx.spectrum_block_ex(n_fft, hop, sig, T, ch, n_streams, d_o.ptr, F * ch * B)
    out = d_o.download()[: n_streams * F * ch * B].reshape(n_streams, F, ch, B)
    d_x.free(); d_o.free()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n_fft", SIZES)
def test_bit_exact_against_the_restatement(ctx, nae, ref, n_fft):
    rng = np.random.default_rng(n_fft + 1)
    for hop in sorted({1, 7, n_fft // 4, n_fft // 2, n_fft}):
        T = n_fft + 40 if hop == 1 else 3 * n_fft + 123
        for ch in (1, 2):
            x = rng.uniform(-1, 1, (2, T * ch)).astype(np.float32)
            got = gpu_ex(ctx, nae, n_fft, hop, x, ch, n_streams=2)
            for s in range(2):
                assert same_bits(got[s], ref_spectrum(ref, x[s], ch, n_fft, hop)), (n_fft, hop, ch, s)


def test_defaults_are_the_1024_point_kernels(ctx, nae):
    rng = np.random.default_rng(11)
    T = 9000
    for ch in (1, 2):
        x = rng.uniform(-1, 1, (3, T * ch)).astype(np.float32)
        F = ctx.spectrum_frames(T)
        d_x = ctx.array(x)
        outs = []
        for any_kernel in (0, 1):
            ctx.debug_set("spec_any", any_kernel)
            for ex in (False, True):
                d_o = ctx.empty(3 * F * ch * 513)
                sig = nae.Sig.interleaved(d_x.ptr, T, ch)
                if ex:
                    ctx.spectrum_block_ex(1024, 256, sig, T, ch, 3, d_o.ptr, F * ch * 513)
                else:
                    ctx.spectrum_block(sig, T, ch, 3, d_o.ptr, F * ch * 513)
                outs.append(d_o.download())
                d_o.free()
        ctx.debug_set("spec_any", 0)
        d_x.free()
        for o in outs[1:]:
            assert same_bits(o, outs[0]), ch
        want = np.stack([orc.spectrum(x[s], ch) for s in range(3)]).reshape(-1)
        assert same_bits(outs[0], want)
    with pytest.raises(nae.NaeError):
        ctx.debug_set("spec_any", 2)


@pytest.mark.parametrize("n_fft", (256, 4096))
def test_hop_invariance(ctx, nae, n_fft):
    rng = np.random.default_rng(5)
    T = n_fft + 7 * 40
    x = rng.uniform(-1, 1, T * 2).astype(np.float32)
    h1 = gpu_ex(ctx, nae, n_fft, 1, x, 2)[0]
    h7 = gpu_ex(ctx, nae, n_fft, 7, x, 2)[0]
    assert h7.shape[0] == 41
    assert same_bits(h7, h1[::7])


@pytest.mark.parametrize("n_fft", (256, 2048))
def test_layouts_streams_and_channels(ctx, nae, n_fft):
    rng = np.random.default_rng(n_fft)
    hop, ch, S, B = n_fft // 4 + 3, 2, 3, bins(n_fft)
    T = 4 * n_fft + 11
    x = rng.uniform(-1, 1, (S, T * ch)).astype(np.float32)
    F = ctx.spectrum_frames_ex(T, n_fft, hop)
    clean = gpu_ex(ctx, nae, n_fft, hop, x, ch, n_streams=S)
    assert same_bits(gpu_ex(ctx, nae, n_fft, hop, x, ch, n_streams=S, planar=True), clean)
    for s in range(S):                                                    # batched == lone runs
        assert same_bits(gpu_ex(ctx, nae, n_fft, hop, x[s], ch)[0], clean[s])
        for c in range(ch):                                               # stereo == two mono runs
            assert same_bits(gpu_ex(ctx, nae, n_fft, hop, x[s].reshape(T, ch)[:, c], 1)[0][:, 0], clean[s][:, c])
    # stream_stride 0: every stream reads stream 0
    d_x = ctx.array(x[0])
    stride = F * ch * B + 5                                               # odd stream stride
    for off in (1, 3):                                                    # odd dst offsets
        d_o = ctx.empty(off + S * stride)
        ctx.spectrum_block_ex(n_fft, hop, nae.Sig(d_x.ptr, 0, 1, ch), T, ch, S, d_o.at(off), stride)
        o = d_o.download()
        for s in range(S):
            assert same_bits(o[off + s * stride: off + s * stride + F * ch * B].reshape(F, ch, B), clean[0]), (off, s)
        d_o.free()
    d_x.free()
    # planar with an odd plane stride and an odd stream stride
    ps, ss = T + 3, 2 * (T + 3) + 1
    host = np.zeros(S * ss, np.float32)
    for s in range(S):
        for c in range(ch):
            host[s * ss + c * ps: s * ss + c * ps + T] = x[s].reshape(T, ch)[:, c]
    d_x, d_o = ctx.array(host), ctx.empty(S * F * ch * B)
    ctx.spectrum_block_ex(n_fft, hop, nae.Sig(d_x.ptr, ss, ps, 1), T, ch, S, d_o.ptr, F * ch * B)
    assert same_bits(d_o.download().reshape(S, F, ch, B), clean)
    d_x.free(); d_o.free()


def test_non_finite_input_stays_in_its_frames(ctx, nae):
    n_fft, hop = 512, 100
    rng = np.random.default_rng(9)
    T = 8 * n_fft
    x = rng.uniform(-1, 1, T * 2).astype(np.float32)
    clean = gpu_ex(ctx, nae, n_fft, hop, x, 2)[0]
    for i, bad in ((1500, np.nan), (3001, np.inf)):
        y = x.copy()
        y[2 * i] = bad                                                    # channel 0 of sample-frame i
        got = gpu_ex(ctx, nae, n_fft, hop, y, 2)[0]
        hit = [f for f in range(clean.shape[0]) if f * hop <= i < f * hop + n_fft]
        for f in range(clean.shape[0]):
            if f in hit:
                assert not np.all(np.isfinite(got[f, 0])), f
            else:
                assert same_bits(got[f, 0], clean[f, 0]), f
            assert same_bits(got[f, 1], clean[f, 1]), f


@pytest.mark.parametrize("n_fft,hop", ((4096, 1000), (256, 64)))
def test_streaming_handle_equals_the_block_call(ctx, nae, n_fft, hop):
    lib = ctx.lib
    ch, B = 2, bins(n_fft)
    rng = np.random.default_rng(hop)
    T = 6 * n_fft + 777
    x = rng.uniform(-1, 1, T * ch).astype(np.float32)
    want = gpu_ex(ctx, nae, n_fft, hop, x, ch)[0]
    h = C.c_void_p()
    assert lib.nae_spectrum_create(ctx.h, n_fft, hop, ch, C.byref(h)) == 0
    d_x = ctx.array(x)
    d_o = ctx.empty(want.size + ch * B)
    cuts = [1, 1, 5, n_fft - 3, 1, hop, 2 * n_fft + 1, 1, 333]
    pos, got_frames, i = 0, 0, 0
    while pos < T:
        n = min(cuts[i % len(cuts)], T - pos)
        i += 1
        assert lib.nae_spectrum_put(h, C.c_void_p(d_x.at(pos * ch)), n) == 0
        pos += n
        avail = lib.nae_spectrum_available(h)
        take = (avail + 1) // 2 if i % 2 else avail                       # partial receives too
        got = C.c_size_t()
        assert lib.nae_spectrum_receive(h, C.c_void_p(d_o.at(got_frames * ch * B)), take, C.byref(got)) == 0
        assert got.value == take
        got_frames += got.value
    rest = lib.nae_spectrum_available(h)
    got = C.c_size_t()
    assert lib.nae_spectrum_receive(h, C.c_void_p(d_o.at(got_frames * ch * B)), rest, C.byref(got)) == 0
    got_frames += got.value
    assert lib.nae_spectrum_destroy(h) == 0
    assert got_frames == want.shape[0]
    out = d_o.download()[: want.size].reshape(want.shape)
    d_x.free(); d_o.free()
    assert same_bits(out, want)


def test_handle_and_block_reject_bad_parameters(ctx, nae):
    lib = ctx.lib
    h = C.c_void_p()
    assert lib.nae_spectrum_create(ctx.h, 2048, 512, 2, C.byref(h)) == 0
    assert lib.nae_spectrum_destroy(h) == 0
    for n, hop, rc in ((128, 32, -2), (8192, 1024, -2), (1000, 250, -2), (1024, 0, -1), (1024, 1025, -1), (4096, 4097, -1)):
        assert lib.nae_spectrum_create(ctx.h, n, hop, 2, C.byref(h)) == rc, (n, hop)
    d = ctx.empty(8192)
    sig = nae.Sig.interleaved(d.ptr, 4096, 2)
    assert lib.nae_spectrum_block_ex_f32(ctx.h, 128, 32, C.byref(sig), 4096, 2, 1, C.c_void_p(d.ptr), 0) == -2
    assert lib.nae_spectrum_block_ex_f32(ctx.h, 512, 0, C.byref(sig), 4096, 2, 1, C.c_void_p(d.ptr), 0) == -1
    assert lib.nae_spectrum_block_ex_f32(ctx.h, 512, 128, C.byref(sig), 4096, 3, 1, C.c_void_p(d.ptr), 0) == -1
    d.free()


def test_host_node_at_4096_hop_512(tmp_path):
    """source -> spectrum {"fft_size": 4096, "hop": 512} -> sink equals the block call, pts advance by hop / sample_rate"""
    import subprocess
    exe = node_harness.build("spec_sizes/host_spectrum.cpp", str(tmp_path))
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "HOST SPECTRUM OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
