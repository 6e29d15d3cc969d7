// host_echo_node.cpp — the host mirror's echo node (tests/test_echo_cpu.py and tests/test_gpu_echo.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_echo round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the eight existing registration calls and after register_echo_processors().
// `gpu`: a source -> audio_echo -> sink graph delivers the frames it received, with their sizes and pts, and the samples of
// nae_echo_block_f32 with the designed parameters, bit for bit: stereo ping-pong with two delays and both loop filters, and mono.
// `short`: a delay under 1024 samples at the stream's rate fails the run on the first frame.  `nyquist`: so does a corner at or above half the
// sample rate.
#include "../node_harness.hpp"
#include "processor/audio-echo.hpp"
#include "nae_dsp_spec.h"

static Json::Value one_key(const char* key, const Json::Value& v)
{
	Json::Value j;
	j[key] = v;
	return j;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_echo node;
	node.deserialize(one_key("delay_ms", 120.0));
	return rejects(node, v, field) && node.delay_ms == 120.0 && !node.delay_ms_right.has_value() && node.feedback == Audio_echo::default_feedback;
}

static void test_json()
{
	Audio_echo node;
	CHECK(node.delay_ms == 350 && !node.delay_ms_right.has_value() && node.feedback == 0.4 && !node.ping_pong && node.damp_hz == 0 && node.lowcut_hz == 0 &&
			  node.wet == 0.35 && node.dry == 1,
		  "defaults 350 ms / no right delay / 0.4 / no ping-pong / no corners / 0.35 / 1");
	CHECK(node.serialize().isNull(), "defaults: nothing written");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull(), "a project without the keys is the default node");
	{
		Json::Value v;
		v["delay_ms"] = 125.5;
		v["delay_ms_right"] = 250.25;
		v["feedback"] = 0.75;
		v["ping_pong"] = true;
		v["damp_hz"] = 4000;
		v["lowcut_hz"] = 150;
		v["wet"] = 0.5;
		v["dry"] = 0.25;
		Audio_echo a, c;
		a.deserialize(v);
		CHECK(a.delay_ms == 125.5 && a.delay_ms_right.has_value() && *a.delay_ms_right == 250.25 && a.feedback == 0.75 && a.ping_pong && a.damp_hz == 4000 &&
				  a.lowcut_hz == 150 && a.wet == 0.5 && a.dry == 0.25,
			  "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 8 && w["delay_ms"].asDouble() == 125.5 && w["delay_ms_right"].asDouble() == 250.25 && w["feedback"].asDouble() == 0.75 &&
				  w["ping_pong"].asBool() && w["damp_hz"].asDouble() == 4000 && w["lowcut_hz"].asDouble() == 150 && w["wet"].asDouble() == 0.5 &&
				  w["dry"].asDouble() == 0.25,
			  "every key written");
		c.deserialize(w);
		CHECK(c.delay_ms == 125.5 && *c.delay_ms_right == 250.25 && c.feedback == 0.75 && c.ping_pong && c.damp_hz == 4000 && c.lowcut_hz == 150 && c.wet == 0.5 &&
				  c.dry == 0.25,
			  "round trip");
		// a later project without the keys brings the defaults back, the right delay included
		c.deserialize(Json::Value());
		CHECK(c.serialize().isNull() && !c.delay_ms_right.has_value(), "absent keys are the defaults");
	}
	{
		// only what differs from the defaults is written; a right delay is written whenever it was given, the left one's value included
		Audio_echo a;
		a.deserialize(one_key("delay_ms_right", 350.0));
		const Json::Value w = a.serialize();
		CHECK(w.size() == 1 && w["delay_ms_right"].asDouble() == 350.0, "a given right delay is kept and written");
		Audio_echo b;
		b.deserialize(one_key("wet", 1.0));
		CHECK(b.serialize().size() == 1 && b.serialize()["wet"].asDouble() == 1.0, "only non-defaults written");
		Audio_echo c;
		c.deserialize(one_key("ping_pong", false));
		CHECK(c.serialize().isNull(), "ping_pong false is the default");
	}
	for (const char* key : {"delay_ms", "delay_ms_right"})
	{
		for (double d : {0.0, -5.0, 2e9}) CHECK(rejects_keeping(one_key(key, d), key), key << " " << d << " rejected");
		CHECK(rejects_keeping(one_key(key, "long"), key) && rejects_keeping(one_key(key, true), key), key << ": a string and a bool rejected");
	}
	for (double g : {-0.1, 0.96, 1.0, 5.0}) CHECK(rejects_keeping(one_key("feedback", g), "feedback"), "feedback " << g << " rejected");
	for (double hz : {-1.0, 1.0, 199.0, 20001.0}) CHECK(rejects_keeping(one_key("damp_hz", hz), "damp_hz"), "damp_hz " << hz << " rejected");
	for (double hz : {-1.0, 1.0, 19.5, 2000.5}) CHECK(rejects_keeping(one_key("lowcut_hz", hz), "lowcut_hz"), "lowcut_hz " << hz << " rejected");
	for (const char* key : {"wet", "dry"})
		for (double v : {-0.01, 1.01}) CHECK(rejects_keeping(one_key(key, v), key), key << " " << v << " rejected");
	for (const char* key : {"feedback", "damp_hz", "lowcut_hz", "wet", "dry"}) CHECK(rejects_keeping(one_key(key, "much"), key), key << ": a string rejected");
	CHECK(rejects_keeping(one_key("ping_pong", 1), "ping_pong") && rejects_keeping(one_key("ping_pong", "yes"), "ping_pong"), "ping_pong: a number and a string rejected");
	{
		Json::Value lo, hi;
		lo["feedback"] = 0.0; lo["damp_hz"] = 200; lo["lowcut_hz"] = 20; lo["wet"] = 0.0; lo["dry"] = 0.0;
		hi["feedback"] = 0.95; hi["damp_hz"] = 20000; hi["lowcut_hz"] = 2000; hi["wet"] = 1.0; hi["dry"] = 1.0;
		Audio_echo a;
		a.deserialize(lo);
		CHECK(a.feedback == 0 && a.damp_hz == 200 && a.lowcut_hz == 20 && a.wet == 0 && a.dry == 0, "the lower limits are accepted");
		a.deserialize(hi);
		CHECK(a.feedback == 0.95 && a.damp_hz == 20000 && a.lowcut_hz == 2000 && a.wet == 1 && a.dry == 1, "the upper limits are accepted");
		Json::Value zero;
		zero["damp_hz"] = 0; zero["lowcut_hz"] = 0;
		a.deserialize(zero);
		CHECK(a.damp_hz == 0 && a.lowcut_hz == 0, "a corner of 0 is none");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_echo a;
		a.feedback = 2; a.damp_hz = 50; a.lowcut_hz = 5000; a.wet = -1; a.dry = 3; a.delay_ms = -4; a.delay_ms_right = 0.0;
		CHECK(a.draw_content(false) == false && a.feedback == 0.95 && a.damp_hz == 200 && a.lowcut_hz == 2000 && a.wet == 0 && a.dry == 1 && a.delay_ms == 1 &&
				  *a.delay_ms_right == 1,
			  "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_echo"); }

static void graph_case(int channels, const Json::Value& json, double delay_s_left, double delay_s_right, double feedback, double damp_hz, double lowcut_hz,
					   double wet, double dry, int cross, const char* what)
{
	const int S = 40000, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_echo>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_echo -> sink runs: " << error);
	if (!ok) return;
	nae_echo_params params;
	CHECK(nae_echo_design(48000, delay_s_left, delay_s_right, feedback, damp_hz, lowcut_hz, wet, dry, cross, &params) == 0, "design");
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_echo_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	check_frames(*sink, y, S, frame_size, what, channels);
}

static void test_gpu()
{
	{
		// 3000 and 4500 samples at 48 kHz: repeats cross 13 chunks and the two lines differ
		Json::Value v;
		v["delay_ms"] = 62.5;
		v["delay_ms_right"] = 93.75;
		v["feedback"] = 0.6;
		v["ping_pong"] = true;
		v["damp_hz"] = 3000;
		v["lowcut_hz"] = 200;
		v["wet"] = 0.5;
		v["dry"] = 0.75;
		graph_case(2, v, 0.0625, 0.09375, 0.6, 3000, 200, 0.5, 0.75, 1, "stereo ping-pong: the block call's samples with the designed parameters");
	}
	{
		// the right delay absent: the left one's; the other keys at their defaults
		Json::Value v;
		v["delay_ms"] = 25.0;
		graph_case(2, v, 0.025, 0.025, 0.4, 0, 0, 0.35, 1, 0, "stereo defaults at 25 ms: the block call's samples");
		graph_case(1, v, 0.025, 0.025, 0.4, 0, 0, 0.35, 1, 0, "mono defaults at 25 ms: the block call's samples");
	}
}

static void expect_failure(const Json::Value& json, const char* needle, const char* what)
{
	const std::vector<float> x = uniform_noise(4000);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_echo>(x, json, 1152, sink, &error);
	CHECK(!ok && error.find(needle) != std::string::npos, what << ": " << error);
}

static void test_short()
{
	// 21 ms at 48 kHz are 1008 samples: under one chunk
	expect_failure(one_key("delay_ms", 21.0), "1008 samples", "a delay under 1024 samples fails the run on the first frame");
	Json::Value v;
	v["delay_ms"] = 100.0;
	v["delay_ms_right"] = 30000.0;   // 1 440 000 samples
	expect_failure(v, "30000 ms", "a right delay above 1048576 samples fails the run on the first frame");
}

static void test_nyquist()
{
	Json::Value v;
	v["delay_ms"] = 100.0;
	v["damp_hz"] = 19000;
	std::shared_ptr<Sink> sink;
	std::string error;
	const std::vector<float> x = uniform_noise(4000);
	// 19 kHz at a 32 kHz stream: above Nyquist
	const bool ok = run_graph<Audio_echo>(x, v, 1152, sink, &error, 32000);
	CHECK(!ok && error.find("19000 Hz") != std::string::npos, "a corner above Nyquist fails the run on the first frame: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "ECHO", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"short", test_short}, {"nyquist", test_nyquist}});
}
