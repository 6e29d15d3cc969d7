"""CPU: tests/block_gpu.py's view_call and stream still catch what they are there to catch.  A stand-in context keeps its arrays in host
memory and the block entry is a Python function that walks the two nae_sig structs, so no context is created and no device entry is called: a
correct entry comes back exact in every view; one that writes behind in_len or in front of the destination, or reads outside the source's
signals, is caught.  The put loop runs against a stand-in handle that releases whole units of 16 frames and records its puts and receives:
the switches that defer the receives behind the flush, cut them into pieces and alternate device and host puts do what they say."""
import ctypes as C

import numpy as np
import pytest

from block_gpu import CONFIGS, bits, noise, stream, view_call

N, STREAMS, CH = 37, 3, 2      # the sizes of the wrong entries' cases


class HostArray:
    def __init__(self, host):
        self.buf = np.array(host, np.float32)

    def at(self, k):
        return self.buf.ctypes.data + 4 * k

    @property
    def ptr(self):
        return self.at(0)

    def download(self):
        return self.buf.copy()

    def free(self):
        pass


class HostContext:
    array = staticmethod(HostArray)


def floats(sig):
    """the memory around sig.base, indexed in floats from it (a negative index lies in front)"""
    return C.cast(sig.base, C.POINTER(C.c_float))


def at(sig, s, c, i):
    return s * sig.stream_stride + c * sig.chan_stride + i * sig.frame_stride


def doubling(src, n, ch, n_streams, dst):
    """the correct entry: y = 2 x"""
    x, y = floats(src), floats(dst)
    for s in range(n_streams):
        for c in range(ch):
            for i in range(n):
                y[at(dst, s, c, i)] = 2 * x[at(src, s, c, i)]


def test_a_correct_entry_is_exact_in_every_view(nae):
    rng = np.random.default_rng(1)
    for ch, n_streams, sl, dl, shared in CONFIGS:
        x = noise(rng, n_streams, N, ch, shared)
        got = view_call(nae, HostContext, doubling, x, sl, dl, shared, gap=5, offset=3, chan_pad=3 if "p" in (sl, dl) else 0)
        assert np.array_equal(bits(got), bits(2 * x)), (ch, n_streams, sl, dl, shared)


def writes_behind(src, n, ch, n_streams, dst):
    doubling(src, n, ch, n_streams, dst)
    floats(dst)[at(dst, n_streams - 1, 0, n)] = 1.0


def writes_in_front(src, n, ch, n_streams, dst):
    doubling(src, n, ch, n_streams, dst)
    floats(dst)[-1] = 1.0


def reads_frame_in_len(src, n, ch, n_streams, dst):
    doubling(src, n, ch, n_streams, dst)
    floats(dst)[at(dst, 1, 0, n - 1)] = 2 * floats(src)[at(src, 1, 0, n)]


def reads_the_gap(src, n, ch, n_streams, dst):
    doubling(src, n, ch, n_streams, dst)
    floats(dst)[at(dst, 0, 1, 0)] = 2 * floats(src)[at(src, 1, 0, 0) - 1]


@pytest.mark.parametrize("layout", ("i", "p"))
def test_wrong_entries_are_caught(nae, layout):
    x = noise(np.random.default_rng(2), STREAMS, N, CH)
    views = dict(src_layout=layout, dst_layout=layout, gap=5, offset=3, chan_pad=3 if layout == "p" else 0)
    with pytest.raises(AssertionError, match="wrote behind in_len"):
        view_call(nae, HostContext, writes_behind, x, **views)
    with pytest.raises(AssertionError, match="wrote in front"):
        view_call(nae, HostContext, writes_in_front, x, **views)
    for call in (reads_frame_in_len, reads_the_gap):
        got = view_call(nae, HostContext, call, x, **views)
        assert np.isnan(got).any() and np.count_nonzero(bits(got) != bits(2 * x)) == 1, call.__name__


class UnitHandle:
    """a handle that passes its input on: whole units of 16 frames as they fill, the rest after the flush"""

    def __init__(self, ch):
        self.ch, self.data, self.taken, self.flushed, self.closed = ch, np.zeros(0, np.float32), 0, False, False
        self.puts, self.receives = [], []      # ("host" | "device", frames); (frames, behind the flush)

    def put_host(self, x):
        self.data = np.concatenate([self.data, x])
        self.puts.append(("host", len(x) // self.ch))

    def put(self, dev_ptr, frames):
        x = np.ctypeslib.as_array(C.cast(dev_ptr, C.POINTER(C.c_float)), (frames * self.ch,))
        self.data = np.concatenate([self.data, x])
        self.puts.append(("device", frames))

    def flush(self):
        self.flushed = True

    def available(self):
        n = len(self.data) // self.ch
        return (n if self.flushed else n // 16 * 16) - self.taken

    def receive_host(self, max_frames=None):
        n = self.available() if max_frames is None else min(max_frames, self.available())
        out = self.data[self.taken * self.ch:(self.taken + n) * self.ch]
        self.taken += n
        self.receives.append((n, self.flushed))
        return out

    def receive(self, dev_ptr, max_frames):
        out = self.receive_host(max_frames)
        np.ctypeslib.as_array(C.cast(dev_ptr, C.POINTER(C.c_float)), (max(len(out), 1),))[:len(out)] = out
        return len(out) // self.ch

    def close(self):
        self.closed = True


def test_stream_delivers_the_input_in_whole_units():
    x = noise(np.random.default_rng(3), 1, 150, CH)[0]
    seen, h = [], UnitHandle(CH)

    def on_put(pos, taken, avail):
        seen.append(pos)
        assert taken + avail == pos // 16 * 16

    got = stream(h, None, x, (1, 15, 17, 100), on_put=on_put, after_flush=lambda taken: seen.append(taken))
    assert np.array_equal(bits(got), bits(x)) and h.closed
    assert seen == [1, 16, 33, 133, 150, 144], "the last size is repeated up to the end; after_flush sees what was received before it"


def test_stream_defers_the_receives_behind_the_flush():
    """defer: every put is made and seen by on_put with nothing taken, no receive comes before the flush, and the input comes out whole"""
    x = noise(np.random.default_rng(5), 1, 150, CH)[0]
    seen, h = [], UnitHandle(CH)

    def on_put(pos, taken, avail):
        seen.append((pos, taken, avail))

    got = stream(h, None, x, (1, 15, 17, 100), on_put=on_put, after_flush=lambda taken: seen.append(taken), defer=True)
    assert np.array_equal(bits(got), bits(x)) and h.closed
    assert seen == [(1, 0, 0), (16, 0, 16), (33, 0, 32), (133, 0, 128), (150, 0, 144), 0], "what is available grows; nothing was taken"
    assert h.receives == [(150, True)], "one receive, behind the flush"
    undeferred = UnitHandle(CH)
    stream(undeferred, None, x, (1, 15, 17, 100))
    assert undeferred.receives == [(16, False), (16, False), (96, False), (16, False), (6, True)], "without the switch: after every put that releases"


def test_stream_receives_in_pieces_and_puts_in_turn():
    """piece: no receive takes more, and they go on until nothing is left; a sequence of device flags is taken in turn, put after put"""
    x = noise(np.random.default_rng(6), 1, 150, CH)[0]
    h = UnitHandle(CH)
    got = stream(h, HostContext, x, (150,), device=(True, False), piece=64)
    assert np.array_equal(bits(got), bits(x))
    assert h.puts == [("device", 150)] and h.receives == [(64, False), (64, False), (16, False), (6, True)]
    h, d_out = UnitHandle(CH), HostArray(np.zeros(64 * CH))
    got = stream(h, HostContext, x, (70,), d_out=d_out, piece=64)
    assert np.array_equal(bits(got), bits(x)), "a receive into device memory is read after it was made"
    assert h.receives == [(64, False), (64, False), (16, False), (6, True)]
    h = UnitHandle(CH)
    got = stream(h, HostContext, x, (40, 30), device=(True, False), defer=True, piece=100)
    assert np.array_equal(bits(got), bits(x))
    assert h.puts == [("device", 40), ("host", 30), ("device", 30), ("host", 30), ("device", 20)] and h.receives == [(100, True), (50, True)]


def test_stream_raises_what_on_put_raises():
    x = noise(np.random.default_rng(4), 1, 150, CH)[0]
    h = UnitHandle(CH)

    def on_put(pos, taken, avail):
        assert taken + avail == pos, "everything put is available"

    with pytest.raises(AssertionError, match="everything put is available"):
        stream(h, None, x, (1, 15, 17, 100), on_put=on_put)
    assert h.closed
