// host_lim_node.cpp — the host mirror's limiter node (tests/test_lim_cpu.py and tests/test_gpu_lim.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_limiter round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the fourteen existing registration calls, each with the count it had, and after
// register_limiter_processors().  `gpu`: a source -> audio_limiter -> sink graph delivers the frames it received, with their sizes and pts, and
// the samples of nae_lim_block_f32 with the designed parameters, bit for bit (tests/test_gpu_lim.py holds that entry to the statement); no
// sample lies above the ceiling; a look-ahead too long for the stream's rate fails the run on the first frame.
#include "../node_harness.hpp"
#include "processor/audio-limiter.hpp"
#include "nae_dsp_spec.h"

static const char* real_keys[] = {"ceiling_db", "gain_db", "release_ms", "lookahead_ms"};
static const double real_lo[] = {-20, -24, 1, 0}, real_hi[] = {0, 24, 5000, 20};
static const char* flag_keys[] = {"true_peak", "link_channels"};

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_limiter node;
	node.deserialize(with("gain_db", 7.0));
	return rejects(node, v, field) && node.gain_db == 7 && node.ceiling_db == -1 && node.release_ms == 100 && node.lookahead_ms == 1.5 && node.true_peak &&
		   node.link_channels;
}

static void test_json()
{
	Audio_limiter node;
	CHECK(node.ceiling_db == -1 && node.gain_db == 0 && node.release_ms == 100 && node.lookahead_ms == 1.5 && node.true_peak && node.link_channels,
		  "defaults: -1 dB, 0 dB, 100 ms, 1.5 ms, true peak, linked");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull() && node.lookahead_ms == 1.5, "a project without the keys keeps the defaults");
	{
		Json::Value v;
		v["ceiling_db"] = -0.3;
		v["gain_db"] = 6.5;
		v["release_ms"] = 250.0;
		v["lookahead_ms"] = 5.0;
		v["true_peak"] = false;
		v["link_channels"] = false;
		Audio_limiter a, c;
		a.deserialize(v);
		const auto all = [](const Audio_limiter& s) {
			return s.ceiling_db == -0.3 && s.gain_db == 6.5 && s.release_ms == 250 && s.lookahead_ms == 5 && !s.true_peak && !s.link_channels;
		};
		CHECK(all(a), "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 6 && w["ceiling_db"].asDouble() == -0.3 && w["gain_db"].asDouble() == 6.5 && w["release_ms"].asDouble() == 250 &&
				  w["lookahead_ms"].asDouble() == 5 && w["true_peak"].asBool() == false && w["link_channels"].asBool() == false,
			  "every key written");
		c.deserialize(w);
		CHECK(all(c), "round trip");
		a.deserialize(Json::Value());
		CHECK(a.ceiling_db == -1 && a.gain_db == 0 && a.true_peak && a.link_channels && a.serialize().isNull(), "absent keys are their defaults again");
	}
	{
		Audio_limiter a;
		a.deserialize(with("ceiling_db", -1.0));
		a.deserialize(with("lookahead_ms", 1.5));
		a.deserialize(with("true_peak", true));
		CHECK(a.serialize().isNull(), "the defaults, spelled out, are not written back");
		a.deserialize(with("release_ms", 40.0));
		CHECK(a.serialize().size() == 1 && a.serialize()["release_ms"].asDouble() == 40, "only non-defaults written");
	}
	for (int i = 0; i < 4; i++)
	{
		const char* key = real_keys[i];
		CHECK(rejects_keeping(with(key, real_lo[i] - 0.5), key) && rejects_keeping(with(key, real_hi[i] + 0.5), key), key << ": values outside the range rejected");
		CHECK(rejects_keeping(with(key, "loud"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_limiter a;
		a.deserialize(with(key, real_lo[i]));
		a.deserialize(with(key, real_hi[i]));
		const Json::Value w = a.serialize();
		CHECK(w.size() == 1 && w[key].asDouble() == real_hi[i], key << ": the limits themselves are accepted");
	}
	for (const char* key : flag_keys)
		CHECK(rejects_keeping(with(key, 1), key) && rejects_keeping(with(key, "yes"), key), key << ": a number and a string rejected");
	{
		// the headless draw_content keeps what the widgets would
		Audio_limiter a;
		a.ceiling_db = 3;
		a.gain_db = -60;
		a.release_ms = 0;
		a.lookahead_ms = 50;
		CHECK(a.draw_content(false) == false && a.ceiling_db == 0 && a.gain_db == -24 && a.release_ms == 1 && a.lookahead_ms == 20, "draw_content: values in range");
	}
}

// the fourteen existing calls keep their counts; the fifteenth adds audio_limiter
static void test_registry()
{
	const auto& map = infra::Processor::processor_map;
	for (const Registration& r : registrations)
	{
		r.call();
		CHECK(map.size() == r.count, "behind the call that adds " << (*r.adds ? r.adds : "the reference's list") << ": " << map.size() << " entries, not " << r.count);
	}
	infra::register_multiband_processors();
	CHECK(map.size() == 19 && map.count("audio_multiband") == 1, "audio_multiband behind its call: " << map.size() << " entries");
	infra::register_separation_processors();
	print_registry();
	CHECK(map.size() == 20 && map.count("audio_separation") == 1 && map.count("audio_limiter") == 0, "no audio_limiter before its call: " << map.size() << " entries");
	infra::register_limiter_processors();
	print_registry();
	CHECK(map.size() == 21 && map.count("audio_limiter") == 1, "audio_limiter behind its call: " << map.size() << " entries");
	check_generated("audio_limiter");
}

// noise in stretches of 5000 samples at full scale and at -40 dB, the right channel quieter: the limiter works and rests, and the link matters
static std::vector<float> noise(size_t frames, int channels)
{
	std::vector<float> x = uniform_noise(frames * channels);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < channels; c++)
			x[n * channels + c] = (float)((double)x[n * channels + c] * ((n / 5000) % 2 == 0 ? 1.0 : 0.01) * (c ? 0.4 : 1.0));
	return x;
}

static void graph_case(int channels, const Json::Value& json, double ceiling_db, double gain_db, double release_s, double lookahead_s, int true_peak, int link,
					   const char* what)
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = noise(S, channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_limiter>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_limiter -> sink runs: " << error);
	if (!ok) return;
	nae_lim_params params;
	CHECK(nae_lim_design(48000, ceiling_db, gain_db, release_s, lookahead_s, true_peak, link, &params) == 0, "design");
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_lim_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	const double top = std::pow(10.0, ceiling_db / 20.0) * (1.0 + std::ldexp(1.0, -22));
	size_t above = 0, reduced = 0;
	double largest = 0;
	for (size_t i = 0; i < y.size(); i++)
	{
		above += std::fabs((double)y[i]) > top;
		largest = std::max(largest, std::fabs((double)y[i]));
		reduced += std::fabs((double)y[i]) < 0.95 * std::fabs((double)x[i]) * std::pow(10.0, gain_db / 20.0);
	}
	CHECK(above == 0, "no sample above the ceiling: " << above);
	CHECK(reduced > y.size() / 10 && largest > 0.5 * top, "the graph's parameters limit: " << reduced << " samples reduced, the largest at " << largest);
	check_frames(*sink, y, S, frame_size, what, channels);
}

static void test_gpu()
{
	graph_case(2, Json::Value(), -1, 0, 0.1, 0.0015, 1, 1, "stereo at the defaults: the block call's samples");
	graph_case(1, Json::Value(), -1, 0, 0.1, 0.0015, 1, 1, "mono at the defaults: the block call's samples");
	{
		Json::Value v;
		v["ceiling_db"] = -3.0; v["gain_db"] = 9.0; v["release_ms"] = 20.0; v["lookahead_ms"] = 5.0; v["true_peak"] = false; v["link_channels"] = false;
		graph_case(2, v, -3, 9, 0.02, 0.005, 0, 0, "stereo driven 9 dB, sample peaks, unlinked, 240 samples of look-ahead");
	}
	{
		const std::vector<float> x = noise(4000, 2);
		Json::Value v;
		v["lookahead_ms"] = 20;   // 960 samples at 48 kHz would do; the source below plays at 96 kHz: 1920
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph<Audio_limiter>(x, v, 1152, sink, &error, 96000);
		CHECK(!ok && error.find("lookahead 20 ms") != std::string::npos && error.find("96000 Hz") != std::string::npos,
			  "a look-ahead of 1920 samples fails the run on the first frame: " << error);
	}
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "LIM", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
