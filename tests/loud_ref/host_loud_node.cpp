// host_loud_node.cpp — the host mirror's loudness node (tests/test_loud_cpu.py and tests/test_gpu_loud.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_loudness round-trips, the defaults are not written back, wrong values are rejected with their key.
// `registry`: no GPU — the processor map after the six existing registration calls and after register_mastering_processors().
// `short`: no GPU — a stream under 400 ms passes as it is, frame for frame.  `gpu`: a source -> audio_loudness -> sink graph with frames that
// do not divide the stream delivers the frames it received, with their sizes and pts, and the samples of nae_loud_normalize_f32 on the whole
// stream, bit for bit: from packed float, planar float and packed S16 stereo (the f32 signal the device makes of them), and from a mono
// stream of exactly one gating block.
#include "../node_harness.hpp"
#include "processor/audio-loudness.hpp"
#include "nae_dsp_spec.h"

static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_loudness node;
	Json::Value b;
	b["target_lufs"] = -23;
	node.deserialize(b);
	return rejects(node, v, field) && node.target_lufs == -23 && node.true_peak_db == -1 && node.max_gain_db == 20;
}

static void test_json()
{
	Audio_loudness node;
	CHECK(node.target_lufs == -14 && node.true_peak_db == -1 && node.max_gain_db == 20 && node.serialize().isNull(), "defaults -14 / -1 / 20, nothing written");
	node.deserialize(Json::Value());
	CHECK(node.target_lufs == -14 && node.serialize().isNull(), "a project without the keys has the defaults");
	{
		Json::Value v;
		v["target_lufs"] = -23.5;
		v["true_peak_db"] = -2.25;
		v["max_gain_db"] = 6;
		Audio_loudness a, c;
		a.deserialize(v);
		CHECK(a.target_lufs == -23.5 && a.true_peak_db == -2.25 && a.max_gain_db == 6, "read");
		const Json::Value w = a.serialize();
		CHECK(w["target_lufs"].asDouble() == -23.5 && w["true_peak_db"].asDouble() == -2.25 && w["max_gain_db"].asDouble() == 6, "written");
		c.deserialize(w);
		CHECK(c.target_lufs == -23.5 && c.true_peak_db == -2.25 && c.max_gain_db == 6, "round trip");
		Json::Value one;
		one["true_peak_db"] = -3;
		a.deserialize(one);
		const Json::Value w1 = a.serialize();
		CHECK(a.target_lufs == -14 && a.max_gain_db == 20 && !w1.isMember("target_lufs") && !w1.isMember("max_gain_db") && w1["true_peak_db"].asDouble() == -3,
			  "an absent key is its default; only non-defaults are written");
	}
	struct Range { const char* key; double lo, hi; };
	for (const Range& r : {Range{"target_lufs", -70, -5}, Range{"true_peak_db", -20, 0}, Range{"max_gain_db", 0, 40}})
	{
		for (double bad : {r.lo - 0.5, r.hi + 0.5, 1e9, -1e9})
		{
			Json::Value v;
			v[r.key] = bad;
			CHECK(rejects_keeping(v, r.key), r.key << " " << bad << " rejected, the node as it was");
		}
		Json::Value s, b;
		s[r.key] = "loud";
		b[r.key] = true;
		CHECK(rejects_keeping(s, r.key) && rejects_keeping(b, r.key), r.key << ": a string and a bool rejected");
		for (double ok : {r.lo, r.hi})
		{
			Json::Value v;
			v[r.key] = ok;
			Audio_loudness a;
			a.deserialize(v);
			CHECK((std::string(r.key) == "target_lufs" ? a.target_lufs : std::string(r.key) == "true_peak_db" ? a.true_peak_db : a.max_gain_db) == ok,
				  r.key << ": the limit " << ok << " is accepted");
		}
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_loudness a;
		a.target_lufs = 3;
		a.true_peak_db = -30;
		a.max_gain_db = 100;
		CHECK(a.draw_content(false) == false && a.target_lufs == -5 && a.true_peak_db == -20 && a.max_gain_db == 40, "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_loudness"); }

// the sink's frames are the source's own: sizes, pts and words (check_frames, whose source runs at 48 kHz)
static void test_short()
{
	const int frame_size = 1000;
	for (int S : {19199, 37, 1000})   // one sample short of 400 ms at 48 kHz; less than a frame; exactly one frame
	{
		const std::vector<float> x = uniform_noise((size_t)S * 2, 99 + S);
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph<Audio_loudness>(x, Json::Value(), frame_size, sink, &error);
		CHECK(ok, "a stream of " << S << " samples runs without a GPU: " << error);
		if (ok) check_frames(*sink, x, (size_t)S, frame_size, "under 400 ms: the input's bits");
	}
}

// the f32 signal the node sees of a packed S16 source: nae_to_f32_interleaved on the source's words, in a context of the harness's own
static std::vector<float> s16_seen_as_f32(const std::vector<float>& x, int ch)
{
	const std::vector<int16_t> q = quantise_s16(x.data(), x.size());
	std::vector<float> seen(x.size());
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return {};
	void *d_q = nullptr, *d_f = nullptr;
	CHECK(nae_malloc(ctx, q.size() * sizeof(int16_t), &d_q) == 0 && nae_malloc(ctx, seen.size() * sizeof(float), &d_f) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_q, q.data(), q.size() * sizeof(int16_t)) == 0, "h2d");
	const void* planes[1] = {d_q};
	CHECK(nae_to_f32_interleaved(ctx, AV_SAMPLE_FMT_S16, planes, x.size() / ch, ch, static_cast<float*>(d_f)) == 0, "nae_to_f32_interleaved");
	CHECK(nae_memcpy_d2h(ctx, seen.data(), d_f, seen.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_q);
	nae_free(ctx, d_f);
	nae_ctx_destroy(ctx);
	return seen;
}

// x, S samples of ch channels, leaves a source of `format` in frames of 1000; `seen` is the f32 signal the node has of it.  The sink holds the
// source's frames, sizes and pts, and the samples of nae_loud_normalize_f32 on the whole of `seen`, bit for bit
static void graph_against_the_block_entry(const std::vector<float>& x, const std::vector<float>& seen, int S, int format, int ch, const char* what)
{
	const int frame_size = 1000;
	Json::Value v;
	v["target_lufs"] = -16;
	v["true_peak_db"] = -1.5;
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_loudness>(x, v, frame_size, sink, &error, 48000, format, ch);
	CHECK(ok, what << ": source -> audio_loudness -> sink runs: " << error);
	if (!ok || seen.empty()) return;
	nae_loud_params params;
	CHECK(nae_loud_design(48000, -16, -1.5, 20, &params) == 0, "design");
	const std::vector<float> y = block_call(seen, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) {
		return nae_loud_normalize_f32(ctx, &params, sx, S, ch, 1, sy, nullptr);
	}, ch);
	if (y.empty()) return;
	size_t changed = 0;
	for (size_t i = 0; i < y.size(); i++) changed += y[i] != seen[i];
	CHECK(changed > y.size() / 2, what << ": the gain is not 1: " << changed << " words changed");
	check_frames(*sink, y, S, frame_size, what, ch);
}

static void test_gpu()
{
	// 30037 samples in frames of 1000: 30 whole frames and one of 37, none of them a multiple of a chunk or a sub-block; noise at -30 dB, so
	// the default target asks for gain and the ceiling does not bind
	const int S = 30037;
	std::vector<float> x = uniform_noise((size_t)S * 2);
	for (size_t i = 0; i < x.size(); i++) x[i] *= (i & 1) ? 0.015625f : 0.03125f;
	graph_against_the_block_entry(x, x, S, AV_SAMPLE_FMT_FLT, 2, "the samples of nae_loud_normalize_f32 on the whole stream");
	// converted input: the node keeps what the device made of the frames.  Planar float is the same floats; of packed S16 it is
	// nae_to_f32_interleaved's signal
	graph_against_the_block_entry(x, x, S, AV_SAMPLE_FMT_FLTP, 2, "planar float: nae_loud_normalize_f32 on the same floats");
	graph_against_the_block_entry(x, s16_seen_as_f32(x, 2), S, AV_SAMPLE_FMT_S16, 2, "packed S16: nae_loud_normalize_f32 on the converted words");
	// mono, and exactly one gating block at 48 kHz (one sample more than `short`'s 19199): the handle is made, the gain applied
	const int M = 19200;
	std::vector<float> m = uniform_noise((size_t)M, 77);
	for (float& s : m) s *= 0.03125f;
	graph_against_the_block_entry(m, m, M, AV_SAMPLE_FMT_FLT, 1, "mono, one gating block: nae_loud_normalize_f32 with ch = 1");
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "LOUD", {{"json", test_json}, {"registry", test_registry}, {"short", test_short}, {"gpu", test_gpu}});
}
