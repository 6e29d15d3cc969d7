// host_dither_node.cpp — the host mirror's dither node (tests/test_dither_cpu.py and tests/test_gpu_dither.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_dither round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the fifteen existing registration calls, each with the count it had, and after
// register_dither_processors().  `gpu [dir]`: a source -> audio_dither -> sink graph delivers the frames it received, with their sizes and pts
// (the frame size does not divide the stream: the last frame is short), and the samples of nae_dither_block_f32 with the node's parameters and
// seed, bit for bit; "taps" overrides "shaping"; with a directory the inputs and outputs are written there as raw f32, and
// tests/test_gpu_dither.py holds them to the CPU statement.
#include "../node_harness.hpp"
#include "processor/audio-dither.hpp"
#include "nae_dsp_spec.h"

#include <fstream>

static std::string dump_dir;

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

static Json::Value array_of(std::initializer_list<double> values)
{
	Json::Value a(Json::arrayValue);
	for (double v : values) a.append(v);
	return a;
}

static bool is_default(const Audio_dither& n)
{
	return n.bits == 16 && n.dither == Audio_dither::Dither::Triangular && n.shaping == Audio_dither::Shaping::None && n.taps.empty() && n.seed == 1;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_dither node;
	node.deserialize(with("bits", 20));
	return rejects(node, v, field) && node.bits == 20 && node.dither == Audio_dither::Dither::Triangular && node.shaping == Audio_dither::Shaping::None &&
		   node.taps.empty() && node.seed == 1;
}

static void test_json()
{
	Audio_dither node;
	CHECK(is_default(node), "defaults: 16 bits, triangular, no shaping, no taps, seed 1");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull() && is_default(node), "a project without the keys keeps the defaults");
	{
		Json::Value v;
		v["bits"] = 24;
		v["dither"] = "highpass";
		v["shaping"] = "lipshitz";
		v["taps"] = array_of({1.5, -0.25, 0.125});
		v["seed"] = 123456789012345.0;
		Audio_dither a, c;
		a.deserialize(v);
		const auto all = [](const Audio_dither& s) {
			return s.bits == 24 && s.dither == Audio_dither::Dither::Highpass && s.shaping == Audio_dither::Shaping::Lipshitz &&
				   s.taps == std::vector<double>{1.5, -0.25, 0.125} && s.seed == 123456789012345ull;
		};
		CHECK(all(a), "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 5 && w["bits"].asInt() == 24 && w["dither"].asString() == "highpass" && w["shaping"].asString() == "lipshitz" &&
				  w["taps"].isArray() && w["taps"].size() == 3 && w["taps"][1].asDouble() == -0.25 && w["seed"].asDouble() == 123456789012345.0,
			  "every key written");
		c.deserialize(w);
		CHECK(all(c), "round trip");
		a.deserialize(Json::Value());
		CHECK(is_default(a) && a.serialize().isNull(), "absent keys are their defaults again");
	}
	{
		const char* kinds[] = {"none", "rectangular", "triangular", "highpass"};
		const Audio_dither::Dither kind_values[] = {Audio_dither::Dither::None, Audio_dither::Dither::Rectangular, Audio_dither::Dither::Triangular,
													Audio_dither::Dither::Highpass};
		for (int i = 0; i < 4; i++)
		{
			Audio_dither a;
			a.deserialize(with("dither", kinds[i]));
			const Json::Value w = a.serialize();
			CHECK(a.dither == kind_values[i] && (i == 2 ? w.isNull() : w.size() == 1 && w["dither"].asString() == kinds[i]), "dither " << kinds[i]);
		}
		const char* shapings[] = {"none", "first", "second", "lipshitz"};
		for (int i = 0; i < 4; i++)
		{
			Audio_dither a;
			a.deserialize(with("shaping", shapings[i]));
			const Json::Value w = a.serialize();
			CHECK((int)a.shaping == i && (i == 0 ? w.isNull() : w.size() == 1 && w["shaping"].asString() == shapings[i]), "shaping " << shapings[i]);
		}
	}
	{
		Audio_dither a;
		a.deserialize(with("bits", 16));
		a.deserialize(with("dither", "triangular"));
		a.deserialize(with("shaping", "none"));
		a.deserialize(with("seed", 1));
		CHECK(a.serialize().isNull(), "the defaults, spelled out, are not written back");
		a.deserialize(with("bits", 8));
		CHECK(a.serialize().size() == 1 && a.serialize()["bits"].asInt() == 8, "only non-defaults written");
		a.deserialize(with("bits", 24));
		CHECK(a.bits == 24, "the limits themselves are accepted");
		a.deserialize(with("seed", 0));
		CHECK(a.seed == 0 && a.serialize().size() == 1 && a.serialize()["seed"].asDouble() == 0, "seed 0 is a seed");
		a.deserialize(with("seed", 9007199254740991.0));
		CHECK(a.seed == 9007199254740991ull, "the largest exact seed");
	}
	// bits
	CHECK(rejects_keeping(with("bits", 7), "bits") && rejects_keeping(with("bits", 25), "bits") && rejects_keeping(with("bits", 16.5), "bits"), "bits: outside 8 ... 24 or not an integer rejected");
	CHECK(rejects_keeping(with("bits", "16"), "bits") && rejects_keeping(with("bits", true), "bits"), "bits: a string and a bool rejected");
	// names
	for (const char* key : {"dither", "shaping"})
		CHECK(rejects_keeping(with(key, "blue"), key) && rejects_keeping(with(key, 1), key) && rejects_keeping(with(key, true), key) && rejects_keeping(with(key, ""), key),
			  key << ": an unknown name, a number and a bool rejected");
	CHECK(rejects_keeping(with("dither", "first"), "dither") && rejects_keeping(with("shaping", "triangular"), "shaping"), "a name of the other key rejected");
	// taps
	{
		Audio_dither a;
		a.deserialize(with("taps", array_of({64.0})));
		CHECK(a.taps == std::vector<double>{64.0}, "one tap of 64: the sum's limit itself");
		a.deserialize(with("taps", array_of({1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1})));
		CHECK(a.taps.size() == 12, "twelve taps");
		CHECK(rejects_keeping(with("taps", Json::Value(Json::arrayValue)), "taps"), "taps: an empty array rejected");
		CHECK(rejects_keeping(with("taps", array_of({1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1})), "taps"), "taps: thirteen rejected");
		CHECK(rejects_keeping(with("taps", array_of({64.0, 0.5})), "taps") && rejects_keeping(with("taps", array_of({-40.0, 30.0})), "taps"), "taps: an absolute sum above 64 rejected");
		CHECK(rejects_keeping(with("taps", 1.0), "taps") && rejects_keeping(with("taps", "first"), "taps") && rejects_keeping(with("taps", true), "taps"),
			  "taps: a number, a string and a bool rejected");
		Json::Value mixed(Json::arrayValue);
		mixed.append(1.0);
		mixed.append("x");
		CHECK(rejects_keeping(with("taps", mixed), "taps"), "taps: a string among the numbers rejected");
		Json::Value inf(Json::arrayValue);
		inf.append(std::numeric_limits<double>::infinity());
		CHECK(rejects_keeping(with("taps", inf), "taps"), "taps: a tap that is not finite rejected");
	}
	// seed
	CHECK(rejects_keeping(with("seed", -1), "seed") && rejects_keeping(with("seed", 1.5), "seed") && rejects_keeping(with("seed", 9007199254740992.0), "seed"),
		  "seed: negative, fractional and 2^53 rejected");
	CHECK(rejects_keeping(with("seed", "1"), "seed") && rejects_keeping(with("seed", true), "seed"), "seed: a string and a bool rejected");
	{
		// the headless draw_content keeps what the widgets would
		Audio_dither a;
		a.bits = 40;
		CHECK(a.draw_content(false) == false && a.bits == 24, "draw_content: bits in range");
		a.bits = 2;
		a.draw_content(false);
		CHECK(a.bits == 8, "draw_content: bits in range");
	}
}

// the fifteen existing calls keep their counts; the sixteenth adds audio_dither
static void test_registry()
{
	const auto& map = infra::Processor::processor_map;
	for (const Registration& r : registrations)
	{
		r.call();
		CHECK(map.size() == r.count, "behind the call that adds " << (*r.adds ? r.adds : "the reference's list") << ": " << map.size() << " entries, not " << r.count);
	}
	const size_t listed = map.size();
	if (!map.count("audio_multiband")) infra::register_multiband_processors();
	if (!map.count("audio_separation")) infra::register_separation_processors();
	if (!map.count("audio_limiter")) infra::register_limiter_processors();
	CHECK(listed <= 21 && map.size() == 21 && map.count("audio_limiter") == 1 && map.count("audio_dither") == 0, "no audio_dither before its call: " << map.size() << " entries");
	print_registry();
	infra::register_dither_processors();
	print_registry();
	CHECK(map.size() == 22 && map.count("audio_dither") == 1, "audio_dither behind its call: " << map.size() << " entries");
	check_generated("audio_dither");
}

// noise at -20 dBFS with a fade to silence at the end and a stretch over full scale, the right channel quieter: the dither works on a tail and on clipping
static std::vector<float> noise(size_t frames, int channels)
{
	std::vector<float> x = uniform_noise(frames * channels);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < channels; c++)
		{
			const double fade = n > frames * 3 / 4 ? (double)(frames - n) / (double)(frames / 4) : 1.0;
			const double level = (n / 3000) % 4 == 3 ? 1.2 : 0.1;
			x[n * channels + c] = (float)((double)x[n * channels + c] * level * fade * fade * (c ? 0.4 : 1.0));
		}
	return x;
}

static void dump(const std::string& name, const std::vector<float>& v)
{
	if (dump_dir.empty()) return;
	std::ofstream f(dump_dir + "/" + name + ".f32", std::ios::binary);
	f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
	CHECK(f.good(), "wrote " << name);
}

static void graph_case(const char* name, int channels, const Json::Value& json, const nae_dither_params& params, const char* what)
{
	const int S = 20011, frame_size = 1000;   // 21 frames, the last of 11 samples
	const std::vector<float> x = noise(S, channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_dither>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_dither -> sink runs: " << error);
	if (!ok) return;
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_dither_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	const double scale = std::ldexp(1.0, params.bits - 1);
	size_t off_grid = 0, moved = 0;
	for (size_t i = 0; i < y.size(); i++)
	{
		const double v = (double)y[i] * scale;
		off_grid += v != std::nearbyint(v) || v < -scale || v > scale - 1;
		moved += y[i] != x[i];
	}
	CHECK(off_grid == 0, "every sample on the grid and in range: " << off_grid);
	CHECK(moved > y.size() / 2, "the graph's parameters quantise: " << moved << " samples moved");
	check_frames(*sink, y, S, frame_size, what, channels);
	std::vector<float> got;
	for (const auto& f : sink->frames)
	{
		const Frame_data* d = f->data();
		got.insert(got.end(), reinterpret_cast<const float*>(d->data[0]), reinterpret_cast<const float*>(d->data[0]) + (size_t)d->nb_samples * channels);
	}
	dump(std::string(name) + "_x", x);
	dump(std::string(name) + "_y", got);
}

static nae_dither_params designed(int bits, int kind, int shaping, unsigned long long seed)
{
	nae_dither_params p;
	CHECK(nae_dither_design(bits, kind, shaping, seed, &p) == 0, "design");
	return p;
}

static void test_gpu()
{
	graph_case("defaults2", 2, Json::Value(), designed(16, NAE_DITHER_TRIANGULAR, NAE_DITHER_SHAPE_NONE, 1), "stereo at the defaults: the block call's samples");
	graph_case("defaults1", 1, Json::Value(), designed(16, NAE_DITHER_TRIANGULAR, NAE_DITHER_SHAPE_NONE, 1), "mono at the defaults: the block call's samples");
	{
		Json::Value v;
		v["bits"] = 12; v["dither"] = "highpass"; v["shaping"] = "lipshitz"; v["seed"] = 99;
		graph_case("shaped2", 2, v, designed(12, NAE_DITHER_HIGHPASS, NAE_DITHER_SHAPE_LIPSHITZ, 99), "stereo, 12 bits, highpass dither, lipshitz shaping, seed 99");
	}
	{
		// "taps" overrides "shaping"
		Json::Value v;
		v["bits"] = 24; v["dither"] = "rectangular"; v["shaping"] = "second"; v["taps"] = array_of({1.25, -0.5, 0.125});
		nae_dither_params p = designed(24, NAE_DITHER_RECTANGULAR, NAE_DITHER_SHAPE_NONE, 1);
		p.n_taps = 3;
		p.taps[0] = 1.25; p.taps[1] = -0.5; p.taps[2] = 0.125;
		graph_case("taps2", 2, v, p, "stereo, 24 bits, the node's own three taps in place of the preset");
	}
}

int main(int argc, char** argv)
{
	if (argc > 2) dump_dir = argv[2];
	return harness_main(argc, argv, "DITHER", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
