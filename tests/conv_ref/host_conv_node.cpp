// host_conv_node.cpp — the host mirror's reverb node (tests/test_conv_cpu.py and tests/test_gpu_conv.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_reverb round-trips, the defaults are not written back, wrong values are rejected.  `registry`: no GPU —
// the processor map after register_all_processors(), register_extension_processors() and register_effect_processors().  `gpu`: a source ->
// audio_reverb -> sink graph delivers the frames it received, with their sizes and pts, and the samples of nae_conv_block_f32 with the
// designed per-channel taps, bit for bit.
#include "../node_harness.hpp"
#include "processor/audio-reverb.hpp"

static bool at_defaults(const Audio_reverb& n)
{
	return n.rt60 == 1.5 && n.predelay_ms == 20 && n.wet == 0.3 && n.dry == 1 && n.seed == 1 && n.fft_size == 0;
}

// a rejected value leaves the node at its defaults
static bool rejects(const Json::Value& v, const std::string& field)
{
	Audio_reverb node;
	return rejects(node, v, field) && at_defaults(node);
}

static void test_json()
{
	Audio_reverb node;
	CHECK(at_defaults(node), "defaults 1.5 s / 20 ms / 0.3 / 1 / seed 1 / pick");
	CHECK(node.serialize().isNull(), "defaults are not written");
	node.deserialize(Json::Value());
	CHECK(at_defaults(node) && node.serialize().isNull(), "a project without the keys keeps the defaults");
	for (double rt : {0.1, 1.5, 5.0})
		for (double pre : {0.0, 20.0, 200.0})
			for (int fft : {0, 512, 4096})
			{
				Json::Value v;
				v["rt60"] = rt;
				v["predelay_ms"] = pre;
				v["wet"] = 0.75;
				v["dry"] = 0.5;
				v["seed"] = 77;
				if (fft) v["fft_size"] = fft;
				Audio_reverb a, b;
				a.deserialize(v);
				CHECK(a.rt60 == rt && a.predelay_ms == pre && a.wet == 0.75 && a.dry == 0.5 && a.seed == 77 && a.fft_size == fft, "read " << rt << " / " << pre << " / " << fft);
				const Json::Value w = a.serialize();
				CHECK(w.isMember("rt60") == (rt != 1.5) && w.isMember("predelay_ms") == (pre != 20.0) && w.isMember("wet") && w.isMember("dry") &&
						  w.isMember("seed") && w.isMember("fft_size") == (fft != 0),
					  "only non-defaults written: " << rt << " / " << pre << " / " << fft);
				b.deserialize(w);
				CHECK(b.rt60 == a.rt60 && b.predelay_ms == a.predelay_ms && b.wet == a.wet && b.dry == a.dry && b.seed == a.seed && b.fft_size == a.fft_size, "round trip");
			}
	{
		Json::Value v;
		v["wet"] = 0;
		v["dry"] = 0;
		v["seed"] = 0;
		Audio_reverb a;
		a.deserialize(v);
		CHECK(a.wet == 0 && a.dry == 0 && a.seed == 0, "the lower ends are values");
	}
	struct Range { const char* key; double below, above; };
	for (const Range& r : {Range{"rt60", 0.09, 5.01}, Range{"predelay_ms", -0.1, 200.5}, Range{"wet", -0.01, 1.01}, Range{"dry", -0.01, 1.01}})
	{
		Json::Value s, lo, hi;
		s[r.key] = "much";
		lo[r.key] = r.below;
		hi[r.key] = r.above;
		CHECK(rejects(s, r.key) && rejects(lo, r.key) && rejects(hi, r.key), r.key << ": a string and values outside the range rejected");
	}
	{
		Json::Value s, n, f, big;
		s["seed"] = "one";
		n["seed"] = -1;
		f["seed"] = 1.5;
		big["seed"] = 1e30;
		CHECK(rejects(s, "seed") && rejects(n, "seed") && rejects(f, "seed") && rejects(big, "seed"), "seed: a string, a negative, a fraction and 1e30 rejected");
	}
	for (double n : {0.0, 256.0, 1000.0, 8192.0, 1024.5, -1024.0})
	{
		Json::Value v;
		v["fft_size"] = n;
		CHECK(rejects(v, "fft_size"), "fft_size " << n << " rejected");
	}
	{
		Json::Value s;
		s["fft_size"] = "big";
		CHECK(rejects(s, "fft_size"), "a string fft_size rejected");
	}
	{
		Audio_reverb a;   // the headless draw_content keeps what the widgets would
		a.rt60 = 9;
		a.predelay_ms = -3;
		a.wet = 2;
		a.dry = -1;
		CHECK(a.draw_content(false) == false && a.rt60 == 5 && a.predelay_ms == 0 && a.wet == 1 && a.dry == 0, "draw_content: values inside their ranges");
	}
}

static void test_registry() { check_registry("audio_reverb"); }

static void test_gpu()
{
	// rt60 0.1 s and 5 ms at 48 kHz: 5040 taps, P = 5 at the picked 2048; frames of 1152 samples against blocks of 1024
	const int S = 20000, frame_size = 1152;
	const double rt60 = 0.1, pre_ms = 5, wet = 0.4, dry = 0.9;
	const uint64_t seed = 9;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	Json::Value v;
	v["rt60"] = rt60;
	v["predelay_ms"] = pre_ms;
	v["wet"] = wet;
	v["dry"] = dry;
	v["seed"] = (int)seed;
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_reverb>(x, v, frame_size, sink, &error);
	CHECK(ok, "source -> audio_reverb -> sink runs: " << error);
	if (!ok) return;
	// the block call with the designed per-channel taps
	const int L = nae_conv_reverb_taps(48000, rt60, pre_ms / 1000.0);
	CHECK(L == 240 + 4800, "response length: " << L);
	std::vector<float> taps((size_t)L * 2);
	for (int c = 0; c < 2; c++)
		CHECK(nae_conv_design_reverb(48000, rt60, pre_ms / 1000.0, dry, wet, seed + c, L, taps.data() + (size_t)c * L) == 0, "design");
	const std::vector<float> y = block_call(x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_conv_block_f32(ctx, taps.data(), L, 2, 0, sx, S, 2, 1, sy); });
	if (y.empty()) return;
	check_frames(*sink, y, S, frame_size, "the samples of the block call with channel c's taps from seed + c");
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "CONV", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
