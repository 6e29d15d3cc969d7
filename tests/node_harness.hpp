// node_harness.hpp — what the host node harnesses (tests/pv_ref/host_pv_node.cpp, tests/spec_sizes/host_spectrum.cpp) share: a CHECK that
// counts failures, a source node that plays interleaved stereo f32 in frames of frame_size, a sink node that keeps every frame, and
// rejects<Node>(json, field), true when deserializing json throws "Wrong field: <field>".
#pragma once
#include "infra/runner.hpp"
#include "processor/audio-velocity.hpp"
#include "nae_gpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>

using namespace processor;
using infra::Runner;

static int failures = 0;
#define CHECK(cond, msg)                                                                       \
	do {                                                                                       \
		if (!(cond)) { std::cout << "FAIL " << __LINE__ << ": " << msg << "\n"; failures++; } \
	} while (0)

class Src : public infra::Processor
{
  public:

	std::vector<float> samples;  // interleaved stereo
	int frame_size = 1152, sample_rate = 48000;
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
		const size_t total = samples.size() / 2;
		for (size_t pos = 0; pos < total && !stop_token; pos += frame_size)
		{
			const int n = (int)std::min<size_t>(frame_size, total - pos);
			auto frame = std::make_shared<Audio_frame>();
			Frame_data* f = frame->data();
			f->format = AV_SAMPLE_FMT_FLT;
			f->sample_rate = sample_rate;
			f->nb_samples = n;
			f->ch_layout.nb_channels = 2;
			f->time_base = {1, 1000000};
			f->pts = (int64_t)((start_seconds + double(pos) / sample_rate) * 1000000);
			frame_get_buffer(f, 32);
			std::memcpy(f->data[0], samples.data() + pos * 2, (size_t)n * 2 * sizeof(float));
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
