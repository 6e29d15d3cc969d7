// host_mb_node.cpp — the host mirror's multiband node (tests/test_mb_cpu.py and tests/test_gpu_mb.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_multiband round-trips, the defaults are not written back, wrong values and wrong array lengths are
// rejected with their key.  `registry`: no GPU — the processor map after the twelve existing registration calls, each with the count it had,
// and after register_multiband_processors().  `gpu`: a source -> audio_multiband -> sink graph delivers the frames it received, with their
// sizes and pts, and the words of a nae_mb handle fed in other pieces with the designed parameters; nae_mb_block_f32 gives the same words.
// `rate`: a crossover at or above half the stream's rate, and a look-ahead too long for it, fail the run on the first frame.
#include "../node_harness.hpp"
#include "processor/audio-multiband.hpp"
#include "nae_dsp_spec.h"

static Json::Value one_key(const char* key, const Json::Value& v)
{
	Json::Value j;
	j[key] = v;
	return j;
}

static Json::Value numbers(std::initializer_list<double> values)
{
	Json::Value list(Json::arrayValue);
	for (double v : values) list.append(v);
	return list;
}

// n band objects, band `at` with key = v
static Json::Value bands_with(int n, int at, const char* key, const Json::Value& v)
{
	Json::Value list(Json::arrayValue);
	for (int b = 0; b < n; b++) list.append(b == at ? one_key(key, v) : Json::Value(Json::objectValue));
	return list;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_multiband node;
	Json::Value before;
	before["crossovers"] = numbers({300.0});
	before["lookahead_ms"] = 1.5;
	node.deserialize(before);
	return rejects(node, v, field) && node.crossovers == std::vector<double>{300.0} && node.bands.size() == 2 && node.lookahead_ms == 1.5 && node.link_channels;
}

static void test_json()
{
	Audio_multiband node;
	CHECK(node.crossovers == (std::vector<double>{120.0, 2500.0}) && node.bands.size() == 3 && node.lookahead_ms == 0 && node.link_channels,
		  "defaults 120 and 2500 Hz / three bands / 0 / linked");
	for (const auto& b : node.bands)
		CHECK(b.dynamics.threshold_db == -18 && b.dynamics.ratio == 4 && b.dynamics.knee_db == 6 && b.dynamics.attack_ms == 5 && b.dynamics.release_ms == 100 &&
				  b.dynamics.makeup_db == 0 && !b.mute && !b.bypass,
			  "a band's defaults are audio_dynamics'");
	CHECK(node.serialize().isNull(), "defaults: nothing written");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull(), "a project without the keys is the default node");
	{
		Json::Value v;
		v["crossovers"] = numbers({90.0, 800.0, 5000.0});
		Json::Value list(Json::arrayValue);
		for (int b = 0; b < 4; b++)
		{
			Json::Value band;
			band["threshold_db"] = -30.0 + b;
			band["ratio"] = 2.5 + b;
			band["knee_db"] = 3.0 * b + 1.0;
			band["attack_ms"] = 1.0 + b;
			band["release_ms"] = 60.0 * (b + 1);
			band["makeup_db"] = 1.5 * b - 2.0;
			band["mute"] = b == 1;
			band["bypass"] = b == 2;
			list.append(band);
		}
		v["bands"] = list;
		v["lookahead_ms"] = 2.5;
		v["link_channels"] = false;
		Audio_multiband a, c;
		a.deserialize(v);
		const auto all = [](const Audio_multiband& m) {
			bool ok = m.crossovers == std::vector<double>{90.0, 800.0, 5000.0} && m.bands.size() == 4 && m.lookahead_ms == 2.5 && !m.link_channels;
			for (int b = 0; ok && b < 4; b++)
			{
				const auto& d = m.bands[b].dynamics;
				ok = d.threshold_db == -30.0 + b && d.ratio == 2.5 + b && d.knee_db == 3.0 * b + 1.0 && d.attack_ms == 1.0 + b && d.release_ms == 60.0 * (b + 1) &&
					 d.makeup_db == 1.5 * b - 2.0 && m.bands[b].mute == (b == 1) && m.bands[b].bypass == (b == 2);
			}
			return ok;
		};
		CHECK(all(a), "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 4 && w["crossovers"].size() == 3 && w["crossovers"][2].asDouble() == 5000.0 && w["bands"].size() == 4 && w["lookahead_ms"].asDouble() == 2.5 &&
				  w["link_channels"].asBool() == false,
			  "every key written");
		CHECK(w["bands"][0].size() == 6 && w["bands"][1].size() == 7 && w["bands"][1]["mute"].asBool() && w["bands"][2].size() == 7 && w["bands"][2]["bypass"].asBool() &&
				  w["bands"][3]["ratio"].asDouble() == 5.5,
			  "a band writes what differs from its defaults");
		c.deserialize(w);
		CHECK(all(c), "round trip");
		// a later project without the keys brings the defaults back
		c.deserialize(Json::Value());
		CHECK(c.serialize().isNull() && c.bands.size() == 3 && c.link_channels, "absent keys are the defaults");
	}
	{
		// only what differs from the defaults is written
		Audio_multiband b;
		b.deserialize(one_key("crossovers", numbers({200.0})));
		CHECK(b.bands.size() == 2 && b.serialize().size() == 1 && b.serialize()["crossovers"].size() == 1, "crossovers alone: two default bands, no bands key");
		Audio_multiband c;
		c.deserialize(one_key("crossovers", numbers({120.0, 2500.0})));
		CHECK(c.serialize().isNull(), "the default crossovers are not written");
		Audio_multiband d;
		d.deserialize(one_key("bands", bands_with(3, 1, "mute", true)));
		const Json::Value w = d.serialize();
		CHECK(w.size() == 1 && w["bands"].size() == 3 && w["bands"][0].isNull() && w["bands"][1].size() == 1 && w["bands"][1]["mute"].asBool() && w["bands"][2].isNull(),
			  "one muted band: three objects, one key");
		Audio_multiband e;
		e.deserialize(one_key("bands", bands_with(3, 0, "threshold_db", -18.0)));
		CHECK(e.serialize().isNull(), "bands at their defaults are not written");
		Audio_multiband f;
		f.deserialize(one_key("crossovers", numbers({100, 1000})));
		CHECK(f.crossovers == (std::vector<double>{100.0, 1000.0}), "integers are numbers");
	}
	// the arrays: type, length, order, range
	CHECK(rejects_keeping(one_key("crossovers", 200.0), "crossovers") && rejects_keeping(one_key("crossovers", "low"), "crossovers") &&
			  rejects_keeping(one_key("crossovers", true), "crossovers"),
		  "crossovers: a number, a string and a bool rejected");
	CHECK(rejects_keeping(one_key("crossovers", Json::Value(Json::arrayValue)), "crossovers") && rejects_keeping(one_key("crossovers", numbers({100, 200, 300, 400})), "crossovers"),
		  "crossovers: none and four rejected");
	CHECK(rejects_keeping(one_key("crossovers", numbers({500, 200})), "crossovers") && rejects_keeping(one_key("crossovers", numbers({200, 200})), "crossovers"),
		  "crossovers: descending and equal rejected");
	CHECK(rejects_keeping(one_key("crossovers", numbers({0.0, 200})), "crossovers") && rejects_keeping(one_key("crossovers", numbers({-5.0})), "crossovers") &&
			  rejects_keeping(one_key("crossovers", numbers({2.0e6})), "crossovers"),
		  "crossovers: zero, negative and absurd rejected");
	{
		Json::Value mixed(Json::arrayValue);
		mixed.append(100.0);
		mixed.append("high");
		CHECK(rejects_keeping(one_key("crossovers", mixed), "crossovers"), "crossovers: a string among them rejected");
	}
	CHECK(rejects_keeping(one_key("bands", 3), "bands") && rejects_keeping(one_key("bands", "all"), "bands"), "bands: a number and a string rejected");
	// without a crossovers key the default pair stands: three bands
	CHECK(rejects_keeping(one_key("bands", bands_with(2, 0, "mute", true)), "bands") && rejects_keeping(one_key("bands", bands_with(4, 0, "mute", true)), "bands") &&
			  rejects_keeping(one_key("bands", Json::Value(Json::arrayValue)), "bands"),
		  "bands: an array shorter or longer than crossovers + 1 rejected (the default crossovers: three)");
	{
		Json::Value v;
		v["crossovers"] = numbers({300.0});
		v["bands"] = bands_with(3, 0, "mute", true);
		CHECK(rejects_keeping(v, "bands"), "three bands on one crossover rejected");
		v["bands"] = bands_with(2, 0, "mute", true);
		Audio_multiband a;
		a.deserialize(v);
		CHECK(a.bands.size() == 2 && a.bands[0].mute && !a.bands[1].mute, "two bands on one crossover");
		Json::Value list(Json::arrayValue);
		list.append(Json::Value(Json::objectValue));
		list.append(5.0);
		v["bands"] = list;
		CHECK(rejects_keeping(v, "bands"), "a band that is a number rejected");
	}
	// a band's keys: audio_dynamics' ranges
	const struct { const char* key; double below, above, lo, hi; } ranges[] = {
		{"threshold_db", -60.5, 0.5, -60, 0}, {"ratio", 0.9, 100.5, 1, 100}, {"knee_db", -0.1, 24.5, 0, 24}, {"attack_ms", -0.1, 500.5, 0, 500},
		{"release_ms", 0.9, 5000.5, 1, 5000}, {"makeup_db", -24.5, 24.5, -24, 24}};
	for (const auto& r : ranges)
	{
		for (double d : {r.below, r.above}) CHECK(rejects_keeping(one_key("bands", bands_with(3, 2, r.key, d)), r.key), r.key << " " << d << " rejected");
		CHECK(rejects_keeping(one_key("bands", bands_with(3, 0, r.key, "much")), r.key) && rejects_keeping(one_key("bands", bands_with(3, 1, r.key, true)), r.key),
			  r.key << ": a string and a bool rejected");
		for (double d : {r.lo, r.hi})
		{
			Audio_multiband a;
			a.deserialize(one_key("bands", bands_with(3, 1, r.key, d)));
			CHECK(a.bands.size() == 3, r.key << " " << d << " accepted");
		}
	}
	for (const char* key : {"mute", "bypass"})
		CHECK(rejects_keeping(one_key("bands", bands_with(3, 1, key, 1)), key) && rejects_keeping(one_key("bands", bands_with(3, 1, key, "yes")), key),
			  key << ": a number and a string rejected");
	for (double d : {-0.1, 20.5}) CHECK(rejects_keeping(one_key("lookahead_ms", d), "lookahead_ms"), "lookahead_ms " << d << " rejected");
	CHECK(rejects_keeping(one_key("lookahead_ms", "much"), "lookahead_ms") && rejects_keeping(one_key("lookahead_ms", true), "lookahead_ms"),
		  "lookahead_ms: a string and a bool rejected");
	CHECK(rejects_keeping(one_key("link_channels", 1), "link_channels") && rejects_keeping(one_key("link_channels", "yes"), "link_channels"),
		  "link_channels: a number and a string rejected");
	{
		Audio_multiband a;
		a.deserialize(one_key("lookahead_ms", 20.0));
		CHECK(a.lookahead_ms == 20, "the upper limit is accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_multiband a;
		a.crossovers = {5000.0, 0.0, 300.0, 9000.0, 12000.0};
		a.bands.resize(1);
		a.bands[0].dynamics.threshold_db = 3;
		a.bands[0].dynamics.ratio = 500;
		a.lookahead_ms = 50;
		CHECK(a.draw_content(false) == false && a.crossovers == (std::vector<double>{1.0, 300.0, 5000.0}) && a.bands.size() == 4 && a.bands[0].dynamics.threshold_db == 0 &&
				  a.bands[0].dynamics.ratio == 100 && a.lookahead_ms == 20,
			  "draw_content: at most three ascending crossovers in range, one band more, values in range");
	}
}

// the twelve existing calls keep their counts; the thirteenth adds audio_multiband
static void test_registry()
{
	const auto& map = infra::Processor::processor_map;
	for (const Registration& r : registrations)
	{
		r.call();
		CHECK(map.size() == r.count, "behind the call that adds " << (*r.adds ? r.adds : "the reference's list") << ": " << map.size() << " entries, not " << r.count);
	}
	print_registry();
	CHECK(map.size() == 18 && map.count("audio_multiband") == 0, "no audio_multiband before its call: " << map.size() << " entries");
	infra::register_multiband_processors();
	print_registry();
	CHECK(map.size() == 19 && map.count("audio_multiband") == 1, "audio_multiband behind its call: " << map.size() << " entries");
	check_generated("audio_multiband");
}

// noise in stretches of 5000 samples at -6 dB and at -46 dB, the right channel quieter: every band's compressor works and rests, and the link matters
static std::vector<float> noise(size_t frames, int channels)
{
	std::vector<float> x = uniform_noise(frames * channels);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < channels; c++)
			x[n * channels + c] = (float)((double)x[n * channels + c] * ((n / 5000) % 2 == 0 ? 0.5 : 0.005) * (c ? 0.4 : 1.0));
	return x;
}

struct Band_design { double threshold_db, ratio, knee_db, attack_s, release_s, makeup_db; };

// x through a nae_mb handle in puts of `piece` frames -> every frame it hands out
static std::vector<float> through_handle(const nae_mb_params& params, const std::vector<float>& x, size_t S, int channels, size_t piece)
{
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return {};
	nae_mb* h = nullptr;
	CHECK(nae_mb_create(ctx, &params, channels, &h) == 0, "nae_mb_create");
	std::vector<float> y;
	const auto take = [&] {
		std::vector<float> part(nae_mb_available(h) * channels);
		size_t got = 0;
		if (part.empty()) return;
		CHECK(nae_mb_receive_host(h, part.data(), part.size() / channels, &got) == 0 && got == part.size() / channels, "receive");
		y.insert(y.end(), part.begin(), part.end());
	};
	for (size_t pos = 0; pos < S && h; pos += piece)
	{
		CHECK(nae_mb_put_host(h, x.data() + pos * channels, std::min(piece, S - pos)) == 0, "put");
		take();
	}
	if (h)
	{
		CHECK(nae_mb_flush(h) == 0, "flush");
		take();
		nae_mb_destroy(h);
	}
	nae_ctx_destroy(ctx);
	return y;
}

static void graph_case(int channels, const Json::Value& json, const std::vector<double>& crossovers, const std::vector<Band_design>& bands, double lookahead_s, int link,
					   unsigned mute_mask, unsigned bypass_mask, const char* what)
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = noise(S, channels);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_multiband>(x, json, frame_size, sink, &error, 48000, AV_SAMPLE_FMT_FLT, channels);
	CHECK(ok, "source -> audio_multiband -> sink runs: " << error);
	if (!ok) return;
	nae_dyn_params band_params[NAE_MB_MAX_BANDS];
	for (size_t b = 0; b < bands.size(); b++)
		CHECK(nae_dyn_design(48000, bands[b].threshold_db, bands[b].ratio, bands[b].knee_db, bands[b].attack_s, bands[b].release_s, lookahead_s, bands[b].makeup_db, link,
							 &band_params[b]) == 0,
			  "band design");
	nae_mb_params params;
	CHECK(nae_mb_design(48000, (int)bands.size(), crossovers.data(), band_params, mute_mask, bypass_mask, &params) == 0, "design");
	const std::vector<float> ys = through_handle(params, x, S, channels, 777);
	CHECK(ys.size() == (size_t)S * channels, "the handle hands out what it was given: " << ys.size() / channels << " frames");
	if (ys.size() != (size_t)S * channels) return;
	size_t changed = 0;
	for (size_t i = 0; i < ys.size(); i++) changed += std::fabs(ys[i] - x[i]) > 0.05f * std::fabs(x[i]);
	CHECK(changed > ys.size() / 50, "the graph's parameters compress: " << changed << " samples changed by more than a twentieth");
	check_frames(*sink, ys, S, frame_size, what, channels);
	const std::vector<float> y = block_call(
		x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_mb_block_f32(ctx, &params, sx, S, channels, 1, sy); }, channels);
	if (y.empty()) return;
	CHECK(std::memcmp(y.data(), ys.data(), ys.size() * sizeof(float)) == 0, "the block call has the handle's words");
}

static void test_gpu()
{
	const Band_design d{-18, 4, 6, 0.005, 0.1, 0};
	graph_case(2, Json::Value(), {120, 2500}, {d, d, d}, 0, 1, 0, 0, "stereo at the defaults: the handle's samples");
	graph_case(1, Json::Value(), {120, 2500}, {d, d, d}, 0, 1, 0, 0, "mono at the defaults: the handle's samples");
	{
		Json::Value v;
		v["crossovers"] = numbers({90.0, 800.0, 5000.0});
		Json::Value list(Json::arrayValue);
		std::vector<Band_design> bands;
		for (int b = 0; b < 4; b++)
		{
			Json::Value band;
			band["threshold_db"] = -40.0 + 3 * b;
			band["ratio"] = 2.0 + 2 * b;
			band["knee_db"] = 3.0 * b;
			band["attack_ms"] = 1.0 + b;
			band["release_ms"] = 40.0 * (b + 1);
			band["makeup_db"] = 3.0 - b;
			band["mute"] = b == 3;
			band["bypass"] = b == 1;
			list.append(band);
			bands.push_back({-40.0 + 3 * b, 2.0 + 2 * b, 3.0 * b, (1.0 + b) / 1000.0, 40.0 * (b + 1) / 1000.0, 3.0 - b});
		}
		v["bands"] = list;
		v["lookahead_ms"] = 2.5;
		v["link_channels"] = false;
		graph_case(2, v, {90, 800, 5000}, bands, 2.5 / 1000.0, 0, 8, 2, "stereo, four bands, unlinked, with a look-ahead, a muted and a bypassed band");
	}
}

static void test_rate()
{
	const std::vector<float> x = noise(4000, 2);
	{
		std::shared_ptr<Sink> sink;
		std::string error;
		// 4000 Hz is a crossover at 48 kHz; the source below plays at 8 kHz, whose half it is
		const bool ok = run_graph<Audio_multiband>(x, one_key("crossovers", numbers({200.0, 4000.0})), 1152, sink, &error, 8000);
		CHECK(!ok && error.find("4000 Hz at 8000 Hz") != std::string::npos, "a crossover at half the rate fails the run on the first frame: " << error);
	}
	{
		std::shared_ptr<Sink> sink;
		std::string error;
		// 960 samples at 48 kHz would do; the source below plays at 96 kHz: 1920
		const bool ok = run_graph<Audio_multiband>(x, one_key("lookahead_ms", 20), 1152, sink, &error, 96000);
		CHECK(!ok && error.find("lookahead 20 ms") != std::string::npos && error.find("96000 Hz") != std::string::npos,
			  "a look-ahead of 1920 samples fails the run on the first frame: " << error);
	}
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "MB", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"rate", test_rate}});
}
