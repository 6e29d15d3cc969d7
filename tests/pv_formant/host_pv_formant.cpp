// host_pv_formant.cpp — the host mirror's "formant" key of Pitch_modifier (tests/test_pv_formant_cpu.py, json) and a source -> Pitch_modifier
// {"pitch": 4, "formant": true} -> sink graph through the fiber runner against the block call nae_stretch_block_formant_f32 with the node's
// lifter (tests/test_gpu_pv_formant.py, gpu).  Built by its tests with the flags of tests/host/Makefile.
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

	static Info get_processor_info() { return {"formant_test_source", "Source", false, [] { return std::unique_ptr<Processor>(new Src); }, ""}; }
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

	static Info get_processor_info() { return {"formant_test_sink", "Sink", false, [] { return std::unique_ptr<Processor>(new Sink); }, ""}; }
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

static bool rejects(const Json::Value& v)
{
	Pitch_modifier node;
	try
	{
		node.deserialize(v);
	}
	catch (const infra::Processor::Runtime_error& e)
	{
		return e.detail == "Wrong field: formant";
	}
	return false;
}

static void test_json()
{
	Pitch_modifier node;
	CHECK(!node.serialize().isMember("formant"), "a default node writes no formant");
	Json::Value v;
	v["pitch"] = 4.0;
	v["formant"] = true;
	Pitch_modifier a;
	a.deserialize(v);
	const Json::Value w = a.serialize();
	CHECK(w.isMember("formant") && w["formant"].isBool() && w["formant"].asBool(), "true is written back");
	Pitch_modifier b;
	b.deserialize(w);
	CHECK(b.serialize()["formant"].asBool(), "round trip");
	Json::Value off;
	off["formant"] = false;
	Pitch_modifier c;
	c.deserialize(off);
	CHECK(!c.serialize().isMember("formant"), "false is not written");
	Pitch_modifier d;
	d.deserialize(v);
	d.deserialize(Json::Value());
	CHECK(!d.serialize().isMember("formant"), "a missing key means false");
	for (const Json::Value& bad : {Json::Value(1), Json::Value(0.5), Json::Value("true")})
	{
		Json::Value x;
		x["formant"] = bad;
		CHECK(rejects(x), "a formant that is not a bool is rejected");
	}
	Json::Value combo;
	combo["formant"] = true;
	combo["phase_lock"] = true;
	Pitch_modifier e;
	e.deserialize(combo);
	CHECK(e.serialize()["formant"].asBool() && e.serialize()["phase_lock"].asBool(), "combines with phase_lock");
	combo["phase_lock"] = false;
	combo["fft_size"] = 2048;
	Pitch_modifier f;
	f.deserialize(combo);
	CHECK(f.serialize()["formant"].asBool() && f.serialize()["fft_size"].asInt() == 2048, "combines with fft_size");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["formant"] = true;
	Pitch_modifier g;
	g.deserialize(st);
	CHECK(g.serialize()["formant"].asBool() && g.serialize()["algorithm"].asString() == "soundtouch", "kept with the soundtouch algorithm");
	Json::Value vel;
	vel["formant"] = true;
	Velocity_modifier h;
	h.deserialize(vel);
	CHECK(!h.serialize().isMember("formant"), "Velocity_modifier has no formant key");
}

static void test_gpu(const char* out_path)
{
	const int S = 60000, N = 1024;
	const float semis = 4.0f;
	std::vector<float> x((size_t)S * 2);
	uint64_t st = 777;
	for (auto& v : x)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		v = (float)((double)(st >> 40) / (double)(1ull << 24) - 0.5);
	}
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto pitch = std::make_shared<Pitch_modifier>();
	Json::Value v;
	v["pitch"] = (double)semis;
	v["formant"] = true;
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(+4, formant) -> sink runs: " << r.get_processor_resources().at(2)->error_text);
	if (!ok) return;
	std::vector<float> got;
	for (auto& f : sink->frames)
	{
		const Frame_data* d = f->data();
		CHECK(d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == 2, "interleaved stereo f32 out");
		const float* p = reinterpret_cast<const float*>(d->data[0]);
		got.insert(got.end(), p, p + (size_t)d->nb_samples * 2);
	}
	const float pf = std::pow(2.0f, semis / 12.0f);  // what Pitch_modifier passes
	const int lifter = nae_stretch_formant_lifter(48000, N);
	CHECK(lifter == 68, "lifter at 48 kHz: " << lifter);
	nae_stretch_plan pl;
	CHECK(nae_stretch_plan_make_n(1.0, (double)pf, N, S, &pl) == 0, "plan");
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, pl.out_len * 2 * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig si{d_x, (size_t)S * 2, 1, 2}, so{d_o, pl.out_len * 2, 1, 2};
	CHECK(nae_stretch_block_formant_f32(ctx, 1.0, (double)pf, 0u, N, lifter, &si, S, 2, 1, &so) == 0, "block_formant");
	std::vector<float> ref(pl.out_len * 2);
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to the formant block call");
	FILE* fo = std::fopen(out_path, "wb");
	CHECK(fo != nullptr, "open " << out_path);
	if (fo)
	{
		std::fwrite(x.data(), sizeof(float), x.size(), fo);
		std::fwrite(got.data(), sizeof(float), got.size(), fo);
		std::fclose(fo);
	}
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "json";
	if (mode == "json") test_json();
	else if (mode == "gpu" && argc > 2) test_gpu(argv[2]);
	else { std::cout << "usage: host_pv_formant json | gpu <out.f32>\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV FORMANT OK " << mode << "\n";
	return 0;
}
