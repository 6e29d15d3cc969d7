// host_dyn_node.cpp — the host mirror's dynamics node (tests/test_dyn_cpu.py and tests/test_gpu_dyn.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_dynamics round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the four existing registration calls and after register_dynamics_processors().  `gpu`: a
// source -> audio_dynamics -> sink graph delivers the frames it received, with their sizes and pts, and the samples of nae_dyn_block_f32 with
// the designed parameters, bit for bit.  `lookahead`: a look-ahead of more than 1024 samples at the stream's rate fails the run on the first
// frame.
#include "../node_harness.hpp"
#include "processor/audio-dynamics.hpp"
#include "nae_dsp_spec.h"

using Mode = Audio_dynamics::Mode;

static const char* real_keys[] = {"threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "lookahead_ms", "makeup_db"};

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_dynamics node;
	Json::Value b;
	b["ratio"] = 7;
	node.deserialize(b);
	return rejects(node, v, field) && node.ratio == 7 && node.mode == Mode::Compressor && node.threshold_db == -18;
}

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

static void test_json()
{
	Audio_dynamics node;
	CHECK(node.mode == Mode::Compressor && node.threshold_db == -18 && node.ratio == 4 && node.knee_db == 6 && node.attack_ms == 5 && node.release_ms == 100 &&
			  node.lookahead_ms == 0 && node.makeup_db == 0 && node.link_channels,
		  "defaults: compressor, -18 dB, 4:1, knee 6 dB, 5 ms, 100 ms, no look-ahead, no make-up, linked");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull() && node.ratio == 4, "a project without the keys keeps the defaults");
	{
		Json::Value v;
		v["mode"] = "limiter";
		v["threshold_db"] = -3.5;
		v["ratio"] = 20;
		v["knee_db"] = 0;
		v["attack_ms"] = 0.25;
		v["release_ms"] = 250;
		v["lookahead_ms"] = 1.5;
		v["makeup_db"] = 2.25;
		v["link_channels"] = false;
		Audio_dynamics a, c;
		a.deserialize(v);
		CHECK(a.mode == Mode::Limiter && a.threshold_db == -3.5 && a.ratio == 20 && a.knee_db == 0 && a.attack_ms == 0.25 && a.release_ms == 250 &&
				  a.lookahead_ms == 1.5 && a.makeup_db == 2.25 && !a.link_channels,
			  "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 9 && w["mode"].asString() == "limiter" && w["threshold_db"].asDouble() == -3.5 && w["ratio"].asDouble() == 20 &&
				  w["knee_db"].asDouble() == 0 && w["attack_ms"].asDouble() == 0.25 && w["release_ms"].asDouble() == 250 &&
				  w["lookahead_ms"].asDouble() == 1.5 && w["makeup_db"].asDouble() == 2.25 && w["link_channels"].isBool() && !w["link_channels"].asBool(),
			  "every key written");
		c.deserialize(w);
		CHECK(c.mode == a.mode && c.threshold_db == a.threshold_db && c.ratio == a.ratio && c.knee_db == a.knee_db && c.attack_ms == a.attack_ms &&
				  c.release_ms == a.release_ms && c.lookahead_ms == a.lookahead_ms && c.makeup_db == a.makeup_db && c.link_channels == a.link_channels,
			  "round trip");
		a.deserialize(Json::Value());
		CHECK(a.mode == Mode::Compressor && a.ratio == 4 && a.link_channels && a.serialize().isNull(), "absent keys are their defaults again");
	}
	{
		Audio_dynamics a;
		a.deserialize(with("mode", "compressor"));
		a.deserialize(with("link_channels", true));
		CHECK(a.serialize().isNull(), "the defaults, spelled out, are not written back");
		a.deserialize(with("knee_db", 12));
		CHECK(a.serialize().size() == 1 && a.serialize()["knee_db"].asDouble() == 12, "only non-defaults written");
	}
	CHECK(rejects_keeping(with("mode", 1), "mode") && rejects_keeping(with("mode", "expander"), "mode") && rejects_keeping(with("mode", true), "mode"),
		  "mode: a number, an unknown name and a bool rejected");
	CHECK(rejects_keeping(with("link_channels", 1), "link_channels") && rejects_keeping(with("link_channels", "yes"), "link_channels"),
		  "link_channels: a number and a string rejected");
	const double below[] = {-60.5, 0.5, -0.5, -0.5, 0.5, -0.5, -24.5}, above[] = {0.5, 100.5, 24.5, 500.5, 5000.5, 20.5, 24.5};
	const double lo[] = {-60, 1, 0, 0, 1, 0, -24}, hi[] = {0, 100, 24, 500, 5000, 20, 24};
	for (int i = 0; i < 7; i++)
	{
		const char* key = real_keys[i];
		CHECK(rejects_keeping(with(key, below[i]), key) && rejects_keeping(with(key, above[i]), key), key << ": values outside the range rejected");
		CHECK(rejects_keeping(with(key, "loud"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_dynamics a;
		a.deserialize(with(key, lo[i]));
		a.deserialize(with(key, hi[i]));
		CHECK(a.serialize()[key].asDouble() == hi[i] || hi[i] == 0, key << ": the limits themselves are accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_dynamics a;
		a.ratio = 500;
		a.lookahead_ms = 50;
		a.threshold_db = 3;
		CHECK(a.draw_content(false) == false && a.ratio == 100 && a.lookahead_ms == 20 && a.threshold_db == 0, "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_dynamics"); }

// noise whose level swells from far under to over the threshold, the right channel quieter: the link matters
static std::vector<float> noise(size_t frames)
{
	std::vector<float> x = uniform_noise(frames * 2);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < 2; c++) x[n * 2 + c] = (float)((double)x[n * 2 + c] * (0.02 + 0.9 * (double)((n / 500) % 7) / 6.0) * (c ? 0.4 : 1.0));
	return x;
}

static Json::Value graph_json(double lookahead_ms)
{
	Json::Value v;
	v["threshold_db"] = -20;
	v["ratio"] = 6;
	v["knee_db"] = 4;
	v["attack_ms"] = 1.5;
	v["release_ms"] = 60;
	v["lookahead_ms"] = lookahead_ms;
	v["makeup_db"] = 3;
	return v;
}

static void test_gpu()
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = noise(S);
	for (const double lookahead_ms : {0.0, 2.5})
	{
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph<Audio_dynamics>(x, graph_json(lookahead_ms), frame_size, sink, &error);
		CHECK(ok, "source -> audio_dynamics -> sink runs: " << error);
		if (!ok) return;
		// the block call on the same samples with the designed parameters
		nae_dyn_params params;
		CHECK(nae_dyn_design(48000, -20, 6, 4, 0.0015, 0.06, lookahead_ms / 1000.0, 3, 1, &params) == 0 && params.lookahead == (lookahead_ms > 0 ? 120 : 0), "design");
		const std::vector<float> y = block_call(x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_dyn_block_f32(ctx, &params, sx, S, 2, 1, sy); });
		if (y.empty()) return;
		size_t changed = 0;
		for (size_t i = 0; i < y.size(); i++) changed += std::fabs(y[i]) < 0.8f * std::fabs(x[i]);
		CHECK(changed > y.size() / 10, "the graph's parameters compress: " << changed << " samples reduced");
		check_frames(*sink, y, S, frame_size, "the block call's samples with the designed parameters");
	}
}

static void test_lookahead()
{
	const std::vector<float> x = noise(4000);
	Json::Value v;
	v["lookahead_ms"] = 20;   // 960 samples at the source's 48 kHz would do; the source below plays at 96 kHz: 1920
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_dynamics>(x, v, 1152, sink, &error, 96000);
	CHECK(!ok && error.find("lookahead 20 ms at 96000 Hz") != std::string::npos, "a look-ahead of 1920 samples fails the run on the first frame: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "DYN", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"lookahead", test_lookahead}});
}
