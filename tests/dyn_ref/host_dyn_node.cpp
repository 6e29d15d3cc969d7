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

static void print_registry()
{
	std::cout << "REGISTRY";
	for (const auto& [id, info] : infra::Processor::processor_map) std::cout << " " << id;
	std::cout << "\n";
}

static void test_registry()
{
	infra::register_all_processors();
	CHECK(infra::Processor::processor_map.size() == 7, "the reference's list: 7 entries");
	infra::register_extension_processors();
	CHECK(infra::Processor::processor_map.size() == 8, "with the filter: 8");
	infra::register_effect_processors();
	CHECK(infra::Processor::processor_map.size() == 9, "with the reverb: 9");
	infra::register_equalizer_processors();
	print_registry();
	CHECK(infra::Processor::processor_map.size() == 10 && infra::Processor::processor_map.count("audio_dynamics") == 0, "the four existing calls: 10 entries, no audio_dynamics");
	infra::register_dynamics_processors();
	print_registry();
	CHECK(infra::Processor::processor_map.size() == 11 && infra::Processor::processor_map.count("audio_dynamics") == 1, "with the dynamics node: 11 entries");
	if (infra::Processor::processor_map.count("audio_dynamics"))
	{
		const auto node = infra::Processor::processor_map.at("audio_dynamics").generate();
		const auto pins = node->get_pin_attributes();
		CHECK(node->get_processor_info_non_static().identifier == "audio_dynamics" && pins.size() == 2, "generate() gives the node: two pins");
		int inputs = 0;
		for (const auto& p : pins) inputs += p.is_input && p.type.get() == typeid(Audio_stream);
		CHECK(inputs == 1, "one audio input pin, one audio output pin");
	}
}

// noise whose level swells from far under to over the threshold, the right channel quieter: the link matters
static std::vector<float> noise(size_t frames)
{
	std::vector<float> x(frames * 2);
	uint64_t st = 4711;
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < 2; c++)
		{
			st = st * 6364136223846793005ull + 1442695040888963407ull;
			const double u = (double)(st >> 40) / (double)(1ull << 24) * 2.0 - 1.0;
			x[n * 2 + c] = (float)(u * (0.02 + 0.9 * (double)((n / 500) % 7) / 6.0) * (c ? 0.4 : 1.0));
		}
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

// source -> audio_dynamics -> sink; the frames' shapes are checked in check_frames, the samples by the caller
static bool run_graph(const std::vector<float>& x, const Json::Value& json, int frame_size, std::shared_ptr<Sink>& sink, std::string* error = nullptr)
{
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	src->frame_size = frame_size;
	auto dyn = std::make_shared<Audio_dynamics>();
	dyn->deserialize(json);
	sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, dyn); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	if (error) *error = r.get_processor_resources().at(2)->error_text;
	return ok;
}

static void check_frames(const Sink& sink, const std::vector<float>& want, size_t S, int frame_size, const char* what)
{
	const size_t n_frames = (S + frame_size - 1) / frame_size;
	CHECK(sink.frames.size() == n_frames, "as many frames as the source sent: " << sink.frames.size() << " vs " << n_frames);
	size_t pos = 0, bad = 0;
	bool shape_ok = true;
	for (size_t f = 0; f < sink.frames.size(); f++)
	{
		const Frame_data* d = sink.frames[f]->data();
		const int want_n = (int)std::min<size_t>(frame_size, S - std::min<size_t>(S, f * frame_size));
		const int64_t want_pts = (int64_t)((0.5 + double(f * frame_size) / 48000) * 1000000);   // the source's own formula
		shape_ok = shape_ok && d->nb_samples == want_n && d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == 2 && d->sample_rate == 48000 &&
				   d->pts == want_pts && d->time_base.num == 1 && d->time_base.den == 1000000;
		const float* got = reinterpret_cast<const float*>(d->data[0]);
		for (int i = 0; i < d->nb_samples && pos < S; i++, pos++)
			for (int c = 0; c < 2; c++) bad += std::memcmp(&got[i * 2 + c], &want[pos * 2 + c], sizeof(float)) != 0;
	}
	CHECK(shape_ok, "frames of the input's sizes, format FLT, the source's pts and time base");
	CHECK(pos == S, "as many samples as the source sent: " << pos);
	CHECK(bad == 0, what << ": " << bad << " words differ");
}

static void test_gpu()
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = noise(S);
	for (const double lookahead_ms : {0.0, 2.5})
	{
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph(x, graph_json(lookahead_ms), frame_size, sink, &error);
		CHECK(ok, "source -> audio_dynamics -> sink runs: " << error);
		if (!ok) return;
		// the block call on the same samples with the designed parameters, through a context of its own
		nae_dyn_params params;
		CHECK(nae_dyn_design(48000, -20, 6, 4, 0.0015, 0.06, lookahead_ms / 1000.0, 3, 1, &params) == 0 && params.lookahead == (lookahead_ms > 0 ? 120 : 0), "design");
		nae_ctx* ctx = nullptr;
		CHECK(nae_ctx_create(0, &ctx) == 0, "context");
		if (!ctx) return;
		std::vector<float> y((size_t)S * 2);
		void *d_x = nullptr, *d_y = nullptr;
		CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, y.size() * sizeof(float), &d_y) == 0, "malloc");
		CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
		const nae_sig sx{d_x, 0, 1, 2}, sy{d_y, 0, 1, 2};
		CHECK(nae_dyn_block_f32(ctx, &params, &sx, S, 2, 1, &sy) == 0, "block call");
		CHECK(nae_memcpy_d2h(ctx, y.data(), d_y, y.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
		nae_free(ctx, d_x);
		nae_free(ctx, d_y);
		nae_ctx_destroy(ctx);
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
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	src->sample_rate = 96000;
	auto dyn = std::make_shared<Audio_dynamics>();
	dyn->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, dyn); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	const std::string error = r.get_processor_resources().at(2)->error_text;
	CHECK(!ok && error.find("lookahead 20 ms at 96000 Hz") != std::string::npos, "a look-ahead of 1920 samples fails the run on the first frame: " << error);
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "json";
	if (mode == "json") test_json();
	else if (mode == "registry") test_registry();
	else if (mode == "gpu") test_gpu();
	else if (mode == "lookahead") test_lookahead();
	else { std::cout << "usage: host_dyn_node json|registry|gpu|lookahead\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST DYN OK " << mode << "\n";
	return 0;
}
