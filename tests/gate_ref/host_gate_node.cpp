// host_gate_node.cpp — the host mirror's gate node (tests/test_gate_cpu.py and tests/test_gpu_gate.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_gate round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the eleven existing registration calls and after register_gate_processors().
// `gpu`: a source -> audio_gate -> sink graph delivers the frames it received, with their sizes and pts, and the samples of the statement
// (ref_gate.c, compiled into this harness with its flags: -ffp-contract=off) with the designed parameters, bit for bit;
// nae_gate_block_f32 on the same input gives the same words.  `lookahead`: a look-ahead too long for the stream's rate fails the run.
#include "../node_harness.hpp"
#include "processor/audio-gate.hpp"
#include "nae_dsp_spec.h"

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
namespace statement
{
#include "ref_gate.c"
}
#undef T
#undef LANES
#undef C
#undef MAX_LOOKAHEAD
#undef MAX_HOLD
#undef FLOOR_DB

static Json::Value one_key(const char* key, const Json::Value& v)
{
	Json::Value j;
	j[key] = v;
	return j;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_gate node;
	node.deserialize(one_key("range_db", 35.0));
	return rejects(node, v, field) && node.range_db == 35.0 && node.threshold_db == Audio_gate::default_threshold_db && node.hold_ms == Audio_gate::default_hold_ms;
}

static void test_json()
{
	Audio_gate node;
	CHECK(node.mode == Audio_gate::Mode::Gate && node.threshold_db == -40 && node.hysteresis_db == 3 && node.range_db == 60 && node.ratio == 2 && node.attack_ms == 1 &&
			  node.hold_ms == 50 && node.release_ms == 100 && node.lookahead_ms == 0 && node.link_channels,
		  "defaults gate / -40 / 3 / 60 / 2 / 1 ms / 50 ms / 100 ms / 0 / linked");
	CHECK(node.serialize().isNull(), "defaults: nothing written");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull(), "a project without the keys is the default node");
	{
		Json::Value v;
		v["mode"] = "expander";
		v["threshold_db"] = -35.5;
		v["hysteresis_db"] = 6.0;
		v["range_db"] = 24.0;
		v["ratio"] = 3.5;
		v["attack_ms"] = 0.5;
		v["hold_ms"] = 120.0;
		v["release_ms"] = 250.0;
		v["lookahead_ms"] = 2.5;
		v["link_channels"] = false;
		Audio_gate a, c;
		a.deserialize(v);
		const auto all = [](const Audio_gate& g) {
			return g.mode == Audio_gate::Mode::Expander && g.threshold_db == -35.5 && g.hysteresis_db == 6 && g.range_db == 24 && g.ratio == 3.5 && g.attack_ms == 0.5 &&
				   g.hold_ms == 120 && g.release_ms == 250 && g.lookahead_ms == 2.5 && !g.link_channels;
		};
		CHECK(all(a), "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 10 && w["mode"].asString() == "expander" && w["threshold_db"].asDouble() == -35.5 && w["hysteresis_db"].asDouble() == 6 &&
				  w["range_db"].asDouble() == 24 && w["ratio"].asDouble() == 3.5 && w["attack_ms"].asDouble() == 0.5 && w["hold_ms"].asDouble() == 120 &&
				  w["release_ms"].asDouble() == 250 && w["lookahead_ms"].asDouble() == 2.5 && w["link_channels"].asBool() == false,
			  "every key written");
		c.deserialize(w);
		CHECK(all(c), "round trip");
		// a later project without the keys brings the defaults back
		c.deserialize(Json::Value());
		CHECK(c.serialize().isNull() && c.mode == Audio_gate::Mode::Gate && c.link_channels, "absent keys are the defaults");
	}
	{
		// only what differs from the defaults is written
		Audio_gate b;
		b.deserialize(one_key("hold_ms", 10.0));
		CHECK(b.serialize().size() == 1 && b.serialize()["hold_ms"].asDouble() == 10.0, "only non-defaults written");
		Audio_gate c;
		c.deserialize(one_key("mode", "gate"));
		CHECK(c.serialize().isNull(), "mode gate is the default");
		Audio_gate d;
		d.deserialize(one_key("link_channels", true));
		CHECK(d.serialize().isNull(), "linked is the default");
	}
	for (double d : {-90.5, 0.5}) CHECK(rejects_keeping(one_key("threshold_db", d), "threshold_db"), "threshold_db " << d << " rejected");
	for (double d : {-0.1, 24.5}) CHECK(rejects_keeping(one_key("hysteresis_db", d), "hysteresis_db"), "hysteresis_db " << d << " rejected");
	for (double d : {-0.1, 120.5}) CHECK(rejects_keeping(one_key("range_db", d), "range_db"), "range_db " << d << " rejected");
	for (double d : {0.9, 100.5}) CHECK(rejects_keeping(one_key("ratio", d), "ratio"), "ratio " << d << " rejected");
	for (double d : {-0.1, 500.5}) CHECK(rejects_keeping(one_key("attack_ms", d), "attack_ms"), "attack_ms " << d << " rejected");
	for (double d : {-0.1, 10000.5}) CHECK(rejects_keeping(one_key("hold_ms", d), "hold_ms"), "hold_ms " << d << " rejected");
	for (double d : {0.9, 5000.5}) CHECK(rejects_keeping(one_key("release_ms", d), "release_ms"), "release_ms " << d << " rejected");
	for (double d : {-0.1, 20.5}) CHECK(rejects_keeping(one_key("lookahead_ms", d), "lookahead_ms"), "lookahead_ms " << d << " rejected");
	for (const char* key : {"threshold_db", "hysteresis_db", "range_db", "ratio", "attack_ms", "hold_ms", "release_ms", "lookahead_ms"})
		CHECK(rejects_keeping(one_key(key, "much"), key) && rejects_keeping(one_key(key, true), key), key << ": a string and a bool rejected");
	CHECK(rejects_keeping(one_key("mode", "duck"), "mode") && rejects_keeping(one_key("mode", 1), "mode") && rejects_keeping(one_key("mode", true), "mode"),
		  "mode: an unknown name, a number and a bool rejected");
	CHECK(rejects_keeping(one_key("link_channels", 1), "link_channels") && rejects_keeping(one_key("link_channels", "yes"), "link_channels"),
		  "link_channels: a number and a string rejected");
	{
		Json::Value lo, hi;
		lo["threshold_db"] = -90.0; lo["hysteresis_db"] = 0.0; lo["range_db"] = 0.0; lo["ratio"] = 1.0; lo["attack_ms"] = 0.0; lo["hold_ms"] = 0.0;
		lo["release_ms"] = 1.0; lo["lookahead_ms"] = 0.0;
		hi["threshold_db"] = 0.0; hi["hysteresis_db"] = 24.0; hi["range_db"] = 120.0; hi["ratio"] = 100.0; hi["attack_ms"] = 500.0; hi["hold_ms"] = 10000.0;
		hi["release_ms"] = 5000.0; hi["lookahead_ms"] = 20.0;
		Audio_gate a;
		a.deserialize(lo);
		CHECK(a.threshold_db == -90 && a.hysteresis_db == 0 && a.range_db == 0 && a.ratio == 1 && a.attack_ms == 0 && a.hold_ms == 0 && a.release_ms == 1 && a.lookahead_ms == 0,
			  "the lower limits are accepted");
		a.deserialize(hi);
		CHECK(a.threshold_db == 0 && a.hysteresis_db == 24 && a.range_db == 120 && a.ratio == 100 && a.attack_ms == 500 && a.hold_ms == 10000 && a.release_ms == 5000 &&
				  a.lookahead_ms == 20,
			  "the upper limits are accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_gate a;
		a.threshold_db = 3; a.hysteresis_db = 30; a.range_db = 200; a.ratio = 500; a.attack_ms = -1; a.hold_ms = 1e6; a.release_ms = 0; a.lookahead_ms = 50;
		CHECK(a.draw_content(false) == false && a.threshold_db == 0 && a.hysteresis_db == 24 && a.range_db == 120 && a.ratio == 100 && a.attack_ms == 0 && a.hold_ms == 10000 &&
				  a.release_ms == 1 && a.lookahead_ms == 20,
			  "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_gate"); }

// noise in stretches of 5000 samples at -6 dB and at -66 dB, the right channel quieter: the gate opens, holds and closes, and the link matters
static std::vector<float> noise(size_t frames, int channels)
{
	std::vector<float> x = uniform_noise(frames * channels);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < channels; c++)
			x[n * channels + c] = (float)((double)x[n * channels + c] * ((n / 5000) % 2 == 0 ? 0.5 : 0.0005) * (c ? 0.4 : 1.0));
	return x;
}

static void graph_case(int channels, const Json::Value& json, int mode, double threshold_db, double hysteresis_db, double range_db, double ratio, double attack_s,
					   double hold_s, double release_s, double lookahead_s, int link, const char* what)
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = noise(S, channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_gate>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_gate -> sink runs: " << error);
	if (!ok) return;
	nae_gate_params params;
	CHECK(nae_gate_design(48000, mode, threshold_db, hysteresis_db, range_db, ratio, attack_s, hold_s, release_s, lookahead_s, link, &params) == 0, "design");
	statement::ref_gate_params stated;
	static_assert(sizeof(stated) == sizeof(params), "one record");
	std::memcpy(&stated, &params, sizeof(stated));
	std::vector<float> ys((size_t)S * channels);
	CHECK(statement::ref_gate_run(&stated, x.data(), S, channels, ys.data()) == 0, "the statement runs");
	size_t reduced = 0, kept = 0;
	for (size_t i = 0; i < ys.size(); i++)
	{
		reduced += std::fabs(ys[i]) < 0.5f * std::fabs(x[i]);
		kept += ys[i] == x[i] || std::fabs(ys[i]) > 0.99f * std::fabs(x[i]);
	}
	CHECK(reduced > ys.size() / 10 && kept > ys.size() / 10, "the graph's parameters gate: " << reduced << " samples reduced, " << kept << " kept");
	check_frames(*sink, ys, S, frame_size, what, channels);
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_gate_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	CHECK(std::memcmp(y.data(), ys.data(), ys.size() * sizeof(float)) == 0, "the block call has the statement's words");
}

static void test_gpu()
{
	graph_case(2, Json::Value(), NAE_GATE_MODE_GATE, -40, 3, 60, 2, 0.001, 0.05, 0.1, 0, 1, "stereo at the defaults: the statement's samples");
	graph_case(1, Json::Value(), NAE_GATE_MODE_GATE, -40, 3, 60, 2, 0.001, 0.05, 0.1, 0, 1, "mono at the defaults: the statement's samples");
	{
		Json::Value v;
		v["mode"] = "expander"; v["threshold_db"] = -30.0; v["hysteresis_db"] = 6.0; v["range_db"] = 40.0; v["ratio"] = 4.0; v["attack_ms"] = 0.0; v["hold_ms"] = 5.0;
		v["release_ms"] = 20.0; v["lookahead_ms"] = 2.5; v["link_channels"] = false;
		graph_case(2, v, NAE_GATE_MODE_EXPANDER, -30, 6, 40, 4, 0, 0.005, 0.02, 0.0025, 0, "stereo expander, unlinked, with a look-ahead");
	}
}

static void test_lookahead()
{
	const std::vector<float> x = noise(4000, 2);
	Json::Value v;
	v["lookahead_ms"] = 20;   // 960 samples at 48 kHz would do; the source below plays at 96 kHz: 1920
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_gate>(x, v, 1152, sink, &error, 96000);
	CHECK(!ok && error.find("lookahead 20 ms") != std::string::npos && error.find("96000 Hz") != std::string::npos,
		  "a look-ahead of 1920 samples fails the run on the first frame: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "GATE", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"lookahead", test_lookahead}});
}
