"""The named edge cases of the graph step input -> mix(2) -> pitch -> spectrum: tests/test_gpu_graph.py runs every row through
tests/tools/fuzz_graph.run_case, tests/test_fuzz_graph_cpu.py asserts (without a GPU) that every row takes the route, and has the mid_len, its
entry claims.  A row is (id, route, mid_len or None, the record); the route is what the front stage launches:
    fused      mix_resample_tile_kernel
    i2p+rs     amix_i2p_kernel, resample_tile_kernel         generic+rs   amix_generic_kernel, resample_tile_kernel
    i2p        amix_i2p_kernel                               generic      amix_generic_kernel                         none   nothing
Strides are padded up to a multiple of 4 unless the row says otherwise (fuzz_graph.make_case), so a length that is no multiple of 4 reaches the
16-byte routes.  All rows keep S <= 20000 and at most 9 streams."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from fuzz_graph import make_case

ROUTES = {"fused": ("mix_resample_tile_kernel",), "i2p+rs": ("amix_i2p_kernel", "resample_tile_kernel"),
          "generic+rs": ("amix_generic_kernel", "resample_tile_kernel"), "i2p": ("amix_i2p_kernel",), "generic": ("amix_generic_kernel",), "none": ()}
P3, P5, P12 = 2.0 ** (3 / 12), 2.0 ** (5 / 12), 2.0
NAMED = []


def row(name, route, mid_len=None, **kw):
    NAMED.append((name, route, mid_len, make_case(label=name, **kw)))


# ---- a ragged end on the fused route: S = 1, 2, 3 (mod 4), both mix layouts, every occupancy of the four-stream group, in_b shared and per stream
row("ragged-8193-planar-1-stream", "fused", S=8193, n_streams=1, pitch=P3, seed=11)
row("ragged-8194-planar-2-streams-own-b", "fused", S=8194, n_streams=2, pitch=P3, shared_b=False, seed=12)
row("ragged-8195-planar-3-streams", "fused", S=8195, n_streams=3, pitch=P5, seed=13)
row("ragged-3001-planar-4-streams-own-b", "fused", S=3001, n_streams=4, pitch=P3, shared_b=False, seed=14)
row("ragged-8193-interleaved-5-streams", "fused", S=8193, n_streams=5, pitch=P3, planar=False, seed=15)
row("ragged-8194-interleaved-7-streams-own-b", "fused", S=8194, n_streams=7, pitch=P5, planar=False, shared_b=False, seed=16)
row("ragged-3001-interleaved-2-streams-odd-mix-stride", "fused", S=3001, n_streams=2, pitch=P3, planar=False, mix_base=1, mix_pad=3, seed=17)
row("ragged-8195-planar-7-streams-wide-strides", "fused", S=8195, n_streams=7, pitch=P3, shared_b=False, a_base=4, a_pad=4, b_base=8, b_pad=12,
    mix_base=4, plane_pad=8, mix_pad=4, seed=18)
row("ragged-3001-planar-5-streams", "fused", S=3001, n_streams=5, pitch=P3, seed=19)
row("ragged-3002-interleaved-5-streams", "fused", S=3002, n_streams=5, pitch=P3, planar=False, shared_b=False, seed=20)
row("ragged-3003-planar-3-streams", "fused", S=3003, n_streams=3, pitch=P3, shared_b=False, seed=21)
# ---- tile edges: mid_len = tile - 1, tile, tile + 1 and 2 tile, for the 768-frame tile (+3 semitones) and the 512-frame tile (+12)
row("tile-768-minus-1", "fused", 767, S=912, n_streams=5, pitch=P3, seed=31)
row("tile-768", "fused", 768, S=913, n_streams=5, pitch=P3, seed=32)
row("tile-768-plus-1", "fused", 769, S=914, n_streams=5, pitch=P3, planar=False, seed=33)
row("tile-768-twice", "fused", 1536, S=1827, n_streams=2, pitch=P3, seed=34)
row("tile-512-minus-1", "fused", 511, S=1022, n_streams=5, pitch=P12, seed=35)
row("tile-512", "fused", 512, S=1023, n_streams=5, pitch=P12, seed=36)
row("tile-512-plus-1", "fused", 513, S=1025, n_streams=5, pitch=P12, planar=False, seed=37)
row("tile-512-twice", "fused", 1024, S=2047, n_streams=2, pitch=P12, seed=38)
# ---- ratio edges: the tile switch, the fuse limit, just above 1, +12 semitones, and rate != 1 with the transposer first
row("rho-1508-768-last-wide-tile", "fused", S=3003, n_streams=5, pitch=1508 / 768, seed=41)
row("rho-1509-768-first-narrow-tile", "fused", S=3003, n_streams=5, pitch=1509 / 768, seed=41)
row("rho-1508-512-last-fused", "fused", S=3003, n_streams=5, pitch=1508 / 512, seed=42)
row("rho-1509-512-first-unfused", "i2p+rs", S=3003, n_streams=5, pitch=1509 / 512, seed=42)
row("rho-just-above-1", "fused", S=3001, n_streams=3, pitch=1.001, seed=43)
row("rho-plus-12-semitones", "fused", S=8193, n_streams=6, pitch=P12, shared_b=False, seed=44)
row("rate-1.25-pitch-plus-3", "fused", S=3002, n_streams=3, rate=1.25, pitch=P3, seed=45)
row("rate-0.8-pitch-1.5", "fused", S=3003, n_streams=3, rate=0.8, pitch=1.5, planar=False, seed=46)
# ---- tiny: around the 16 taps; a mid_len of 0 still writes the whole mix; S = 0 and no streams leave every sentinel in place
for k, S in enumerate((1, 2, 3, 5, 15, 16, 17, 29)):
    row(f"tiny-{S}", "fused", S=S, n_streams=3, pitch=P3, planar=S not in (5, 17), shared_b=bool(k & 1), seed=50 + k)
row("tiny-1-mid-len-0", "i2p", 0, S=1, n_streams=3, pitch=1508 / 512, seed=58)
row("tiny-3-mid-len-1-five-streams", "fused", 1, S=3, n_streams=5, pitch=1508 / 512, seed=59)
row("empty-length-0", "none", 0, S=0, n_streams=3, pitch=P3, seed=60)
row("empty-no-streams", "none", S=100, n_streams=0, pitch=P3, seed=61)
# ---- fallbacks, taken and still right: each reason the fuse is refused, on the content of ragged-3001-planar-5-streams (seed 19)
row("fallback-in-a-base-1-float-off", "generic+rs", S=3001, n_streams=5, pitch=P3, a_base=1, seed=19)
row("fallback-in-a-base-2-floats-off", "generic+rs", S=3001, n_streams=5, pitch=P3, a_base=2, seed=19)
row("fallback-in-b-base-off", "generic+rs", S=3001, n_streams=5, pitch=P3, b_base=3, seed=19)
row("fallback-in-a-stream-stride-2-mod-4", "generic+rs", S=3001, n_streams=5, pitch=P3, a_pad=2, seed=19)
row("fallback-mix-stream-stride-2-mod-4", "generic+rs", S=3001, n_streams=5, pitch=P3, mix_pad=2, seed=19)
row("fallback-odd-plane-stride", "generic+rs", S=3001, n_streams=5, pitch=P3, plane_pad=1, seed=19)
row("fallback-mix-base-off", "generic+rs", S=3001, n_streams=5, pitch=P3, mix_base=2, seed=19)
row("fallback-rho-past-the-limit", "i2p+rs", S=3001, n_streams=5, pitch=2.0 ** (19 / 12), seed=19)
row("fallback-rho-past-the-limit-interleaved", "generic+rs", S=3002, n_streams=5, pitch=2.0 ** (19 / 12), planar=False, shared_b=False, seed=20)
# ---- volumes: the sign of zero of (0 + a va) + b vb is part of bit-exactness
for k, vols in enumerate(((0.0, 0.0), (0.0, 0.7), (-0.5, 1.0), (1.0, 1.0))):
    row(f"volumes-{vols[0]:g}-{vols[1]:g}", "fused", S=3002, n_streams=2, pitch=P3, vols=vols, planar=bool(k & 1), seed=70)
# ---- pitch output 8 bytes off its 16-byte alignment, padded pitch streams, a gap between the spectrum's streams
row("pitch-out-8-bytes-off", "fused", S=3001, n_streams=5, pitch=P3, pitch_base=2, seed=19)
row("pitch-out-8-bytes-off-padded-streams", "fused", S=3003, n_streams=3, pitch=P3, pitch_base=2, pitch_pad=2, spec_gap=6, seed=21)
row("spectrum-gap-odd", "fused", S=3003, n_streams=3, pitch=P3, pitch_pad=1, spec_gap=1, seed=21)
# ---- the mix as a launch of its own at a ragged length: the vocoder first, the transposer alone, the identity
row("vocoder-first-ragged", "i2p", S=3001, n_streams=5, pitch=2.0 ** (-4 / 12), seed=19)
row("transposer-alone-ragged", "i2p", S=3002, n_streams=3, rate=1.5, pitch=1.0, seed=81)
row("identity-ragged", "i2p", S=3003, n_streams=2, rate=1.0, pitch=1.0, seed=82)
row("vocoder-first-ragged-interleaved", "generic", S=3001, n_streams=2, pitch=2.0 ** (-4 / 12), planar=False, seed=83)

# more streams than one launch of the fused kernel indexes (65535 groups of 4): the front stage alone, tests/tools/fuzz_graph.run_front_only
MANY_STREAMS = [(name, make_case(label=name, S=8, n_streams=65535 * 4 + 3, pitch=P3, planar=planar, shared_b=False, a_pad=4, mix_pad=4, seed=90))
                for name, planar in (("many-streams-planar", True), ("many-streams-interleaved", False))]
