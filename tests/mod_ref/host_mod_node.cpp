// host_mod_node.cpp — the host mirror's modulation node (tests/test_mod_cpu.py and tests/test_gpu_mod.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_modulation round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the nine existing registration calls and after register_modulation_processors().
// `gpu`: a source -> audio_modulation -> sink graph delivers the frames it received, with their sizes and pts, and the samples of
// nae_mod_block_f32 with the designed parameters, bit for bit: the default chorus in stereo and mono, the README's flanger and its vibrato.
// `range`: a delay range outside 2 ... 3070 samples at the stream's rate fails the run on the first frame.
#include "../node_harness.hpp"
#include "processor/audio-modulation.hpp"
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
	Audio_modulation node;
	node.deserialize(one_key("delay_ms", 7.0));
	return rejects(node, v, field) && node.delay_ms == 7.0 && node.voices == Audio_modulation::default_voices && node.feedback == Audio_modulation::default_feedback;
}

static void test_json()
{
	Audio_modulation node;
	CHECK(node.rate_hz == 0.8 && node.delay_ms == 12 && node.depth_ms == 3 && node.feedback == 0 && node.voices == 3 && node.spread == 0.5 &&
			  node.shape == Audio_modulation::Shape::Sine && node.wet == 0.5 && node.dry == 1,
		  "defaults 0.8 Hz / 12 ms / 3 ms / 0 / 3 voices / 0.5 / sine / 0.5 / 1: a chorus");
	CHECK(node.serialize().isNull(), "defaults: nothing written");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull(), "a project without the keys is the default node");
	{
		Json::Value v;
		v["rate_hz"] = 0.25;
		v["delay_ms"] = 3.5;
		v["depth_ms"] = 2.25;
		v["feedback"] = -0.75;
		v["voices"] = 2;
		v["spread"] = 0.125;
		v["shape"] = "triangle";
		v["wet"] = 0.75;
		v["dry"] = 0.25;
		Audio_modulation a, c;
		a.deserialize(v);
		CHECK(a.rate_hz == 0.25 && a.delay_ms == 3.5 && a.depth_ms == 2.25 && a.feedback == -0.75 && a.voices == 2 && a.spread == 0.125 &&
				  a.shape == Audio_modulation::Shape::Triangle && a.wet == 0.75 && a.dry == 0.25,
			  "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 9 && w["rate_hz"].asDouble() == 0.25 && w["delay_ms"].asDouble() == 3.5 && w["depth_ms"].asDouble() == 2.25 &&
				  w["feedback"].asDouble() == -0.75 && w["voices"].asInt() == 2 && w["spread"].asDouble() == 0.125 && w["shape"].asString() == "triangle" &&
				  w["wet"].asDouble() == 0.75 && w["dry"].asDouble() == 0.25,
			  "every key written");
		c.deserialize(w);
		CHECK(c.rate_hz == 0.25 && c.delay_ms == 3.5 && c.depth_ms == 2.25 && c.feedback == -0.75 && c.voices == 2 && c.spread == 0.125 &&
				  c.shape == Audio_modulation::Shape::Triangle && c.wet == 0.75 && c.dry == 0.25,
			  "round trip");
		// a later project without the keys brings the defaults back
		c.deserialize(Json::Value());
		CHECK(c.serialize().isNull() && c.shape == Audio_modulation::Shape::Sine, "absent keys are the defaults");
	}
	{
		// only what differs from the defaults is written
		Audio_modulation b;
		b.deserialize(one_key("wet", 1.0));
		CHECK(b.serialize().size() == 1 && b.serialize()["wet"].asDouble() == 1.0, "only non-defaults written");
		Audio_modulation c;
		c.deserialize(one_key("shape", "sine"));
		CHECK(c.serialize().isNull(), "shape sine is the default");
	}
	for (double r : {-0.1, 20.5, 1000.0}) CHECK(rejects_keeping(one_key("rate_hz", r), "rate_hz"), "rate_hz " << r << " rejected");
	for (double d : {0.0, -5.0, 2e9}) CHECK(rejects_keeping(one_key("delay_ms", d), "delay_ms"), "delay_ms " << d << " rejected");
	for (double d : {-0.5, 2e9}) CHECK(rejects_keeping(one_key("depth_ms", d), "depth_ms"), "depth_ms " << d << " rejected");
	for (double g : {-0.96, 0.96, 1.0, -5.0}) CHECK(rejects_keeping(one_key("feedback", g), "feedback"), "feedback " << g << " rejected");
	for (double n : {0.0, 5.0, -1.0, 2.5}) CHECK(rejects_keeping(one_key("voices", n), "voices"), "voices " << n << " rejected");
	for (const char* key : {"spread", "wet", "dry"})
		for (double v : {-0.01, 1.01}) CHECK(rejects_keeping(one_key(key, v), key), key << " " << v << " rejected");
	for (const char* key : {"rate_hz", "delay_ms", "depth_ms", "feedback", "voices", "spread", "wet", "dry"})
		CHECK(rejects_keeping(one_key(key, "much"), key) && rejects_keeping(one_key(key, true), key), key << ": a string and a bool rejected");
	CHECK(rejects_keeping(one_key("shape", "square"), "shape") && rejects_keeping(one_key("shape", 1), "shape") && rejects_keeping(one_key("shape", true), "shape"),
		  "shape: an unknown name, a number and a bool rejected");
	{
		Json::Value lo, hi;
		lo["rate_hz"] = 0.0; lo["depth_ms"] = 0.0; lo["feedback"] = -0.95; lo["voices"] = 1; lo["spread"] = 0.0; lo["wet"] = 0.0; lo["dry"] = 0.0;
		hi["rate_hz"] = 20.0; hi["feedback"] = 0.95; hi["voices"] = 4; hi["spread"] = 1.0; hi["wet"] = 1.0; hi["dry"] = 1.0;
		Audio_modulation a;
		a.deserialize(lo);
		CHECK(a.rate_hz == 0 && a.depth_ms == 0 && a.feedback == -0.95 && a.voices == 1 && a.spread == 0 && a.wet == 0 && a.dry == 0, "the lower limits are accepted");
		a.deserialize(hi);
		CHECK(a.rate_hz == 20 && a.feedback == 0.95 && a.voices == 4 && a.spread == 1 && a.wet == 1 && a.dry == 1, "the upper limits are accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_modulation a;
		a.rate_hz = 30; a.delay_ms = -4; a.depth_ms = -1; a.feedback = -2; a.voices = 9; a.spread = 3; a.wet = -1; a.dry = 3;
		CHECK(a.draw_content(false) == false && a.rate_hz == 20 && a.delay_ms == 0.05 && a.depth_ms == 0 && a.feedback == -0.95 && a.voices == 4 && a.spread == 1 &&
				  a.wet == 0 && a.dry == 1,
			  "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_modulation"); }

static void graph_case(int channels, const Json::Value& json, double rate_hz, double delay_ms, double depth_ms, double feedback, int voices, double spread,
					   int shape, double wet, double dry, const char* what)
{
	const int S = 40000, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_modulation>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_modulation -> sink runs: " << error);
	if (!ok) return;
	nae_mod_params params;
	CHECK(nae_mod_design(48000, rate_hz, delay_ms, depth_ms, feedback, voices, spread, shape, wet, dry, &params) == 0, "design");
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_mod_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	check_frames(*sink, y, S, frame_size, what, channels);
}

static void test_gpu()
{
	graph_case(2, Json::Value(), 0.8, 12, 3, 0, 3, 0.5, NAE_MOD_SINE, 0.5, 1, "stereo chorus at the defaults: the block call's samples with the designed parameters");
	graph_case(1, Json::Value(), 0.8, 12, 3, 0, 3, 0.5, NAE_MOD_SINE, 0.5, 1, "mono chorus at the defaults: the block call's samples");
	{
		// the README's flanger, on the triangle
		Json::Value v;
		v["delay_ms"] = 3.0; v["depth_ms"] = 2.0; v["rate_hz"] = 0.25; v["feedback"] = 0.7; v["voices"] = 1; v["wet"] = 0.7; v["shape"] = "triangle";
		graph_case(2, v, 0.25, 3, 2, 0.7, 1, 0.5, NAE_MOD_TRIANGLE, 0.7, 1, "stereo flanger: the block call's samples");
	}
	{
		// the README's vibrato
		Json::Value v;
		v["delay_ms"] = 5.0; v["depth_ms"] = 2.0; v["rate_hz"] = 5.0; v["voices"] = 1; v["spread"] = 0.0; v["wet"] = 1.0; v["dry"] = 0.0;
		graph_case(2, v, 5, 5, 2, 0, 1, 0, NAE_MOD_SINE, 1, 0, "stereo vibrato: the block call's samples");
	}
}

static void expect_failure(const Json::Value& json, const char* needle, const char* what)
{
	const std::vector<float> x = uniform_noise(4000);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_modulation>(x, json, 1152, sink, &error);
	CHECK(!ok && error.find(needle) != std::string::npos, what << ": " << error);
}

static void test_range()
{
	// 1 ms less 0.98 ms at 48 kHz are 0.96 samples: under 2
	Json::Value v;
	v["delay_ms"] = 1.0;
	v["depth_ms"] = 0.98;
	expect_failure(v, "delay 1 ms, depth 0.98 ms", "a delay range under 2 samples fails the run on the first frame");
	// 60 ms and 5 ms at 48 kHz reach 3120 samples: above 3070
	Json::Value w;
	w["delay_ms"] = 60.0;
	w["depth_ms"] = 5.0;
	expect_failure(w, "delay 60 ms, depth 5 ms", "a delay range above 3070 samples fails the run on the first frame");
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "MOD", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"range", test_range}});
}
