// host_sat_node.cpp — the host mirror's saturation node (tests/test_sat_cpu.py and tests/test_gpu_sat.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_saturation round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the ten existing registration calls and after register_saturation_processors().
// `gpu`: a source -> audio_saturation -> sink graph delivers the frames it received, with their sizes and pts, and the samples of the
// statement (ref_sat.c, compiled into this harness with its flags: -ffp-contract=off) with the designed parameters on the input extended by
// the latency's zeros, shifted by the latency, bit for bit; nae_sat_block_f32 on the same input gives the same words.
#include "../node_harness.hpp"
#include "processor/audio-saturation.hpp"
#include "nae_dsp_spec.h"

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
namespace statement
{
#include "ref_sat.c"
}
#undef K
#undef MAX_OS
#undef SOFT
#undef HARD
#undef BETA

static Json::Value one_key(const char* key, const Json::Value& v)
{
	Json::Value j;
	j[key] = v;
	return j;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_saturation node;
	node.deserialize(one_key("drive_db", 7.0));
	return rejects(node, v, field) && node.drive_db == 7.0 && node.oversample == Audio_saturation::default_oversample && node.mix == Audio_saturation::default_mix;
}

static void test_json()
{
	Audio_saturation node;
	CHECK(node.drive_db == 12 && node.curve == Audio_saturation::Curve::Soft && node.bias == 0 && node.oversample == 4 && node.output_db == 0 && node.mix == 1,
		  "defaults 12 dB / soft / 0 / 4 / 0 dB / 1");
	CHECK(node.serialize().isNull(), "defaults: nothing written");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull(), "a project without the keys is the default node");
	{
		Json::Value v;
		v["drive_db"] = 24.5;
		v["curve"] = "hard";
		v["bias"] = 0.25;
		v["oversample"] = 8;
		v["output_db"] = -6.5;
		v["mix"] = 0.75;
		Audio_saturation a, c;
		a.deserialize(v);
		CHECK(a.drive_db == 24.5 && a.curve == Audio_saturation::Curve::Hard && a.bias == 0.25 && a.oversample == 8 && a.output_db == -6.5 && a.mix == 0.75, "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 6 && w["drive_db"].asDouble() == 24.5 && w["curve"].asString() == "hard" && w["bias"].asDouble() == 0.25 && w["oversample"].asInt() == 8 &&
				  w["output_db"].asDouble() == -6.5 && w["mix"].asDouble() == 0.75,
			  "every key written");
		c.deserialize(w);
		CHECK(c.drive_db == 24.5 && c.curve == Audio_saturation::Curve::Hard && c.bias == 0.25 && c.oversample == 8 && c.output_db == -6.5 && c.mix == 0.75, "round trip");
		// a later project without the keys brings the defaults back
		c.deserialize(Json::Value());
		CHECK(c.serialize().isNull() && c.curve == Audio_saturation::Curve::Soft, "absent keys are the defaults");
	}
	{
		// only what differs from the defaults is written
		Audio_saturation b;
		b.deserialize(one_key("mix", 0.5));
		CHECK(b.serialize().size() == 1 && b.serialize()["mix"].asDouble() == 0.5, "only non-defaults written");
		Audio_saturation c;
		c.deserialize(one_key("curve", "soft"));
		CHECK(c.serialize().isNull(), "curve soft is the default");
	}
	for (double d : {-0.1, 48.5, 1000.0}) CHECK(rejects_keeping(one_key("drive_db", d), "drive_db"), "drive_db " << d << " rejected");
	for (double b : {-0.01, 1.01}) CHECK(rejects_keeping(one_key("bias", b), "bias"), "bias " << b << " rejected");
	for (double m : {0.0, 3.0, 5.0, 6.0, 7.0, 16.0, -2.0, 2.5}) CHECK(rejects_keeping(one_key("oversample", m), "oversample"), "oversample " << m << " rejected");
	for (double o : {-24.5, 24.5}) CHECK(rejects_keeping(one_key("output_db", o), "output_db"), "output_db " << o << " rejected");
	for (double m : {-0.01, 1.01}) CHECK(rejects_keeping(one_key("mix", m), "mix"), "mix " << m << " rejected");
	for (const char* key : {"drive_db", "bias", "oversample", "output_db", "mix"})
		CHECK(rejects_keeping(one_key(key, "much"), key) && rejects_keeping(one_key(key, true), key), key << ": a string and a bool rejected");
	CHECK(rejects_keeping(one_key("curve", "tube"), "curve") && rejects_keeping(one_key("curve", 1), "curve") && rejects_keeping(one_key("curve", true), "curve"),
		  "curve: an unknown name, a number and a bool rejected");
	{
		Json::Value lo, hi;
		lo["drive_db"] = 0.0; lo["bias"] = 0.0; lo["oversample"] = 1; lo["output_db"] = -24.0; lo["mix"] = 0.0;
		hi["drive_db"] = 48.0; hi["bias"] = 1.0; hi["oversample"] = 8; hi["output_db"] = 24.0; hi["mix"] = 1.0;
		Audio_saturation a;
		a.deserialize(lo);
		CHECK(a.drive_db == 0 && a.bias == 0 && a.oversample == 1 && a.output_db == -24 && a.mix == 0, "the lower limits are accepted");
		a.deserialize(hi);
		CHECK(a.drive_db == 48 && a.bias == 1 && a.oversample == 8 && a.output_db == 24 && a.mix == 1, "the upper limits are accepted");
		for (int m : {1, 2, 4, 8})
		{
			a.deserialize(one_key("oversample", m));
			CHECK(a.oversample == m, "oversample " << m << " accepted");
		}
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_saturation a;
		a.drive_db = 60; a.bias = -1; a.oversample = 5; a.output_db = -30; a.mix = 3;
		CHECK(a.draw_content(false) == false && a.drive_db == 48 && a.bias == 0 && a.oversample == 4 && a.output_db == -24 && a.mix == 1, "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_saturation"); }

static void graph_case(int channels, const Json::Value& json, double drive_db, double bias, int curve, int oversample, double output_db, double mix, const char* what)
{
	const int S = 40000, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_saturation>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_saturation -> sink runs: " << error);
	if (!ok) return;
	nae_sat_params params;
	CHECK(nae_sat_design(drive_db, bias, curve, oversample, output_db, mix, &params) == 0, "design");
	// the statement on the input extended by the latency's zeros; the node drops the latency in front
	const size_t D = (size_t)nae_sat_latency(oversample), T = (size_t)S + D;
	std::vector<float> xz(x);
	xz.resize(T * channels, 0.0f);
	statement::ref_sat_params stated;
	static_assert(sizeof(stated) == sizeof(params), "one record");
	std::memcpy(&stated, &params, sizeof(stated));
	std::vector<float> ys(T * channels);
	CHECK(statement::ref_sat_run(&stated, xz.data(), T, channels, ys.data()) == 0, "the statement runs");
	const std::vector<float> want(ys.begin() + D * channels, ys.end());
	check_frames(*sink, want, S, frame_size, what, channels);
	const std::vector<float> y = block_call(
		xz, T, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_sat_block_f32(ctx, &params, sx, T, channels, 1, sy); }, channels);
	if (y.empty()) return;
	CHECK(std::memcmp(y.data(), ys.data(), ys.size() * sizeof(float)) == 0, "the block call on the extended input has the statement's words");
}

static void test_gpu()
{
	graph_case(2, Json::Value(), 12, 0, NAE_SAT_SOFT, 4, 0, 1, "stereo at the defaults: the block call's samples shifted by the latency");
	graph_case(1, Json::Value(), 12, 0, NAE_SAT_SOFT, 4, 0, 1, "mono at the defaults: the block call's samples shifted by the latency");
	{
		Json::Value v;
		v["drive_db"] = 30.0; v["curve"] = "hard"; v["bias"] = 0.3; v["oversample"] = 8; v["output_db"] = -6.0; v["mix"] = 0.5;
		graph_case(2, v, 30, 0.3, NAE_SAT_HARD, 8, -6, 0.5, "stereo hard clipper at 8x with a bias and a mix");
	}
	{
		Json::Value v;
		v["oversample"] = 2; v["bias"] = 0.1;
		graph_case(1, v, 12, 0.1, NAE_SAT_SOFT, 2, 0, 1, "mono at 2x");
	}
	{
		Json::Value v;
		v["oversample"] = 1; v["drive_db"] = 24.0;
		graph_case(2, v, 24, 0, NAE_SAT_SOFT, 1, 0, 1, "stereo at 1x: no latency");
	}
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "SAT", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
