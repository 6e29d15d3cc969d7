// node_harness.hpp — what the host node harnesses share.  All of them (tests/pv_ref/host_pv_node.cpp, tests/spec_sizes/host_spectrum.cpp and the
// four effect nodes'): a CHECK that counts its evaluations and its failures, a source node that plays interleaved f32 (stereo, packed float
// unless told otherwise) in frames of frame_size, a sink node that keeps every frame, and rejects<Node>(json, field), true when deserializing
// json throws "Wrong field: <field>".
// The effect nodes' (tests/fir_ref/host_fir_node.cpp, conv_ref/host_conv_node.cpp, eq_ref/host_eq_node.cpp, dyn_ref/host_dyn_node.cpp) besides:
// uniform_noise, run_graph<Node> (source -> node -> sink), check_frames (the sink's frames against the source's shapes and the wanted words),
// block_call (a block entry through a context of its own), check_registry (the one walk through the registration calls, with print_registry and
// check_generated), and harness_main (the mode dispatch).
#pragma once
#include "infra/runner.hpp"
#include "processor/audio-velocity.hpp"
#include "nae_gpu.h"

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <iostream>

using namespace processor;
using infra::Runner;

inline int failures = 0;
inline long checks = 0;   // CHECKs evaluated: harness_main prints it, so that a harness that stops checking shows
#define CHECK(cond, msg)                                                                       \
	do {                                                                                       \
		checks++;                                                                              \
		if (!(cond)) { std::cout << "FAIL " << __LINE__ << ": " << msg << "\n"; failures++; } \
	} while (0)

// what a source of format AV_SAMPLE_FMT_S16 sends for x: the nearest of 32767 steps
inline std::vector<int16_t> quantise_s16(const float* x, size_t n)
{
	std::vector<int16_t> q(n);
	for (size_t i = 0; i < n; i++) q[i] = (int16_t)std::lrint(x[i] * 32767.0f);
	return q;
}

class Src : public infra::Processor
{
  public:

	std::vector<float> samples;  // interleaved, `channels` of them
	int frame_size = 1152, sample_rate = 48000;
	int format = AV_SAMPLE_FMT_FLT, channels = 2;  // the frames' format: AV_SAMPLE_FMT_FLT, _FLTP (the planes of samples) or _S16 (quantise_s16 of samples)
	double start_seconds = 0.5;

	static Info get_processor_info() { return {"test_source", "Source", false, [] { return std::unique_ptr<Processor>(new Src); }, ""}; }
	Info get_processor_info_non_static() const override { return get_processor_info(); }
	std::vector<Pin_attribute> get_pin_attributes() const override
	{
		return {{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }}};
	}
	Json::Value serialize() const override { return {}; }
	void deserialize(const Json::Value&) override {}
	void draw_title() override {}
	bool draw_content(bool) override { return false; }
	void process_payload(const std::map<std::string, std::shared_ptr<Product>>&,
						 const std::map<std::string, std::set<std::shared_ptr<Product>>>& output, const std::atomic<bool>& stop_token,
						 std::any&) override
	{
		const auto outs = infra::get_output_item<Audio_stream>(output, "output");
		const size_t total = samples.size() / channels;
		for (size_t pos = 0; pos < total && !stop_token; pos += frame_size)
		{
			const int n = (int)std::min<size_t>(frame_size, total - pos);
			auto frame = std::make_shared<Audio_frame>();
			Frame_data* f = frame->data();
			f->format = format;
			f->sample_rate = sample_rate;
			f->nb_samples = n;
			f->ch_layout.nb_channels = channels;
			f->time_base = {1, 1000000};
			f->pts = (int64_t)((start_seconds + double(pos) / sample_rate) * 1000000);
			frame_get_buffer(f, 32);
			const float* x = samples.data() + pos * channels;
			if (format == AV_SAMPLE_FMT_FLTP)
				for (int c = 0; c < channels; c++)
					for (int i = 0; i < n; i++) reinterpret_cast<float*>(f->data[c])[i] = x[(size_t)i * channels + c];
			else if (format == AV_SAMPLE_FMT_S16)
				std::memcpy(f->data[0], quantise_s16(x, (size_t)n * channels).data(), (size_t)n * channels * sizeof(int16_t));
			else
				std::memcpy(f->data[0], x, (size_t)n * channels * sizeof(float));
			for (auto& o : outs)
				while (!stop_token && o->try_push(frame) != channel_op_status::success) nae_fiber::this_fiber::yield();
		}
		for (auto& o : outs) o->set_eof();
	}
};

class Sink : public infra::Processor
{
  public:

	std::vector<std::shared_ptr<const Audio_frame>> frames;

	static Info get_processor_info() { return {"test_sink", "Sink", false, [] { return std::unique_ptr<Processor>(new Sink); }, ""}; }
	Info get_processor_info_non_static() const override { return get_processor_info(); }
	std::vector<Pin_attribute> get_pin_attributes() const override
	{
		return {{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}};
	}
	Json::Value serialize() const override { return {}; }
	void deserialize(const Json::Value&) override {}
	void draw_title() override {}
	bool draw_content(bool) override { return false; }
	void process_payload(const std::map<std::string, std::shared_ptr<Product>>& input,
						 const std::map<std::string, std::set<std::shared_ptr<Product>>>&, const std::atomic<bool>& stop_token,
						 std::any&) override
	{
		auto in = infra::get_input_item<Audio_stream>(input, "input");
		if (!in.has_value()) throw Runtime_error("sink has no input", "", "");
		Audio_stream& s = in.value().get();
		while (!stop_token)
		{
			auto r = s.try_pop();
			if (!r.has_value())
			{
				if (s.eof()) break;
				nae_fiber::this_fiber::yield();
				continue;
			}
			frames.push_back(r.value());
		}
	}
};

template <class Node>
static bool rejects(Node& node, const Json::Value& v, const std::string& field)
{
	try
	{
		node.deserialize(v);
	}
	catch (const infra::Processor::Runtime_error& e)
	{
		return e.detail == "Wrong field: " + field;
	}
	return false;
}

template <class Node>
static bool rejects(const Json::Value& v, const std::string& field)
{
	Node node;
	return rejects(node, v, field);
}

// n_floats draws from [-1, 1).  Every draw is k / 2^23 - 1 with k < 2^24: exact in float, so shaping it in double loses nothing.
inline std::vector<float> uniform_noise(size_t n_floats, uint64_t seed = 4711)
{
	std::vector<float> x(n_floats);
	for (auto& v : x)
	{
		seed = seed * 6364136223846793005ull + 1442695040888963407ull;
		v = (float)((double)(seed >> 40) / (double)(1ull << 24) * 2.0 - 1.0);
	}
	return x;
}

// source -> Node (deserialized from json) -> sink; the frames' shapes are checked in check_frames, the samples by the caller
template <class Node>
bool run_graph(const std::vector<float>& x, const Json::Value& json, int frame_size, std::shared_ptr<Sink>& sink, std::string* error = nullptr,
			   int sample_rate = 48000, int format = AV_SAMPLE_FMT_FLT, int channels = 2)
{
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	src->frame_size = frame_size;
	src->sample_rate = sample_rate;
	src->format = format;
	src->channels = channels;
	auto node = std::make_shared<Node>();
	node->deserialize(json);
	sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, node); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	if (error) *error = r.get_processor_resources().at(2)->error_text;
	return ok;
}

// the sink holds the frames a 48 kHz source of S samples of ch channels sent, as packed float, and their words are want's
inline void check_frames(const Sink& sink, const std::vector<float>& want, size_t S, int frame_size, const char* what, int ch = 2)
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
		shape_ok = shape_ok && d->nb_samples == want_n && d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == ch && d->sample_rate == 48000 &&
				   d->pts == want_pts && d->time_base.num == 1 && d->time_base.den == 1000000;
		const float* got = reinterpret_cast<const float*>(d->data[0]);
		for (int i = 0; i < d->nb_samples && pos < S; i++, pos++)
			for (int c = 0; c < ch; c++) bad += std::memcmp(&got[i * ch + c], &want[pos * ch + c], sizeof(float)) != 0;
	}
	CHECK(shape_ok, "frames of the input's sizes, format FLT, the source's pts and time base");
	CHECK(pos == S, "as many samples as the source sent: " << pos);
	CHECK(bad == 0, what << ": " << bad << " words differ");
}

// interleaved x of ch channels through a block entry, in a context of its own: call(ctx, &src, &dst) returns the entry's status -> the first
// out_frames frames of the destination; empty when there is no context
template <class Call>
std::vector<float> block_call(const std::vector<float>& x, size_t out_frames, Call call, int ch = 2)
{
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return {};
	std::vector<float> y(out_frames * ch);
	void *d_x = nullptr, *d_y = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, y.size() * sizeof(float), &d_y) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	const nae_sig sx{d_x, 0, 1, (size_t)ch}, sy{d_y, 0, 1, (size_t)ch};
	CHECK(call(ctx, &sx, &sy) == 0, "block call");
	CHECK(nae_memcpy_d2h(ctx, y.data(), d_y, y.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_y);
	nae_ctx_destroy(ctx);
	return y;
}

inline void print_registry()
{
	std::cout << "REGISTRY";
	for (const auto& [id, info] : infra::Processor::processor_map) std::cout << " " << id;
	std::cout << "\n";
}

// what the registry generates for id is that node: two pins, one of them an audio input
inline void check_generated(const std::string& id)
{
	if (!infra::Processor::processor_map.count(id)) return;
	const auto node = infra::Processor::processor_map.at(id).generate();
	const auto pins = node->get_pin_attributes();
	CHECK(node->get_processor_info_non_static().identifier == id && pins.size() == 2, "generate() gives the node: two pins");
	int inputs = 0;
	for (const auto& p : pins) inputs += p.is_input && p.type.get() == typeid(Audio_stream);
	CHECK(inputs == 1, "one audio input pin, one audio output pin");
}

// The registration calls in the order an editor makes them, the node each one adds beyond the reference's seven, and the registry's size behind it.
struct Registration { void (*call)(); const char* adds; size_t count; };
inline const Registration registrations[] = {
	{[] { infra::register_all_processors(); }, "", 7},
	{infra::register_extension_processors, "audio_filter", 8},
	{infra::register_effect_processors, "audio_reverb", 9},
	{infra::register_equalizer_processors, "audio_eq", 10},
	{infra::register_dynamics_processors, "audio_dynamics", 11},
	{infra::register_restoration_processors, "audio_denoise", 12},
	{infra::register_mastering_processors, "audio_loudness", 13},
	{infra::register_sidechain_processors, "audio_sidechain", 14},
	{infra::register_echo_processors, "audio_echo", 15},
	{infra::register_modulation_processors, "audio_modulation", 16},
	{infra::register_saturation_processors, "audio_saturation", 17},
	{infra::register_gate_processors, "audio_gate", 18},
};

// the `registry` mode of a node's harness: the calls up to the one that adds id, the size behind every one of them; id is not there before its
// call and is there behind it, and the registry is printed on both sides of that call (the Python tests read the two lines).  What the
// registry then generates for id is checked by check_generated, or by the harness's own check for a node with other pins.
inline void check_registry(const std::string& id, void (*generated)(const std::string&) = check_generated)
{
	const auto& map = infra::Processor::processor_map;
	for (const Registration& r : registrations)
	{
		const bool adds = id == r.adds;
		if (adds)
		{
			print_registry();
			CHECK(map.count(id) == 0, "no " << id << " before its call");
		}
		r.call();
		CHECK(map.size() == r.count, "behind the call that adds " << (*r.adds ? r.adds : "the reference's list") << ": " << map.size() << " entries, not " << r.count);
		if (!adds) continue;
		print_registry();
		CHECK(map.count(id) == 1, id << " behind its call");
		generated(id);
		return;
	}
	CHECK(false, "no registration call adds " << id);
}

// main() of host_<name>_node: runs the mode argv[1] names ("json" without one) -> 0 and "HOST <NAME> OK <mode>", 1 after a failed CHECK, 2 and
// the usage line for an unknown mode
struct Mode_entry { const char* name; void (*run)(); };
inline int harness_main(int argc, char** argv, const char* name, std::initializer_list<Mode_entry> modes)
{
	const std::string mode = argc > 1 ? argv[1] : "json";
	for (const auto& m : modes)
	{
		if (mode != m.name) continue;
		m.run();
		std::cout << "CHECKS " << checks << "\n";
		if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
		std::cout << "HOST " << name << " OK " << mode << "\n";
		return 0;
	}
	std::cout << "usage: host_";
	for (const char* c = name; *c; c++) std::cout << (char)std::tolower(*c);
	std::cout << "_node";
	for (const auto& m : modes) std::cout << (&m == modes.begin() ? " " : "|") << m.name;
	std::cout << "\n";
	return 2;
}
