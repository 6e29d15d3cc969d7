// host_pv_fshift.cpp — the host mirror's "formant_shift" key on Pitch_modifier (tests/test_pv_fshift_cpu.py, tests/test_gpu_pv_fshift.py).
// Built by its tests with tests/node_harness.py.
//
// `json`: no GPU — absent means 0 and is not written; a number of semitones round-trips (an integer too); 0 is not written; a value that is not
// a number is "Wrong field: formant_shift"; beyond +-24 it is a Runtime_error "Out of range: formant_shift"; it combines with "phase_lock",
// "fft_size", "transients" and "formant"; with "algorithm": "soundtouch" it is kept; Velocity_modifier ignores the key.
// `gpu <pitch> <shift> <in.f32> <out.f32>`: source -> Pitch_modifier {"pitch": <pitch>, "formant_shift": <shift>} -> sink through the fiber
// runner equals nae_stretch_block_formant_shift_f32 (default lifter, formant_ratio 2^(shift / 12)) on the same samples bit for bit, and differs
// from the call without the shift; the input and the graph's output are written for the caller's comparison with the CPU statement.
#include "../node_harness.hpp"
#include <cstdio>
#include <cstdlib>

static bool out_of_range(const Json::Value& v)
{
	Pitch_modifier node;
	try
	{
		node.deserialize(v);
	}
	catch (const infra::Processor::Runtime_error& e)
	{
		return e.detail == "Out of range: formant_shift";
	}
	return false;
}

static void test_json()
{
	Pitch_modifier node;
	CHECK(!node.serialize().isMember("formant_shift"), "a default node writes no formant_shift");
	for (const Json::Value& s : {Json::Value(4.0), Json::Value(-5.0), Json::Value(3), Json::Value(24), Json::Value(-24.0), Json::Value(0.5)})
	{
		Json::Value v;
		v["formant_shift"] = s;
		Pitch_modifier a;
		a.deserialize(v);
		const Json::Value w = a.serialize();
		CHECK(w.isMember("formant_shift") && w["formant_shift"].isDouble() && w["formant_shift"].asFloat() == s.asFloat(), "a shift is written back");
		Pitch_modifier b;
		b.deserialize(w);
		CHECK(b.serialize()["formant_shift"].asFloat() == s.asFloat(), "round trip");
		a.deserialize(Json::Value());
		CHECK(!a.serialize().isMember("formant_shift"), "a missing key means 0");
	}
	Json::Value zero;
	zero["formant_shift"] = 0.0;
	Pitch_modifier z;
	z.deserialize(zero);
	CHECK(!z.serialize().isMember("formant_shift"), "0 is not written");
	for (const Json::Value& bad : {Json::Value(true), Json::Value("4"), Json::Value(false)})
	{
		Json::Value v;
		v["formant_shift"] = bad;
		CHECK(rejects<Pitch_modifier>(v, "formant_shift"), "a formant_shift that is not a number is rejected");
	}
	for (double far : {24.5, -24.01, 100.0, -1e9})
	{
		Json::Value v;
		v["formant_shift"] = far;
		CHECK(out_of_range(v), "a formant_shift beyond +-24 semitones is out of range: " << far);
	}
	Json::Value all;
	all["pitch"] = 0.0;
	all["formant_shift"] = 4.0;
	all["phase_lock"] = true;
	all["transients"] = true;
	all["formant"] = true;
	Pitch_modifier c;
	c.deserialize(all);
	const Json::Value cw = c.serialize();
	CHECK(cw["formant_shift"].asFloat() == 4.0f && cw["phase_lock"].asBool() && cw["transients"].asBool() && cw["formant"].asBool() && cw["pitch"].asFloat() == 0.0f,
		  "combines with phase_lock, transients and formant");
	Json::Value sz;
	sz["formant_shift"] = -3.0;
	sz["fft_size"] = 2048;
	Pitch_modifier d;
	d.deserialize(sz);
	CHECK(d.serialize()["formant_shift"].asFloat() == -3.0f && d.serialize()["fft_size"].asInt() == 2048 && !d.serialize().isMember("formant"),
		  "combines with fft_size, and does not set formant");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["formant_shift"] = 2.0;
	Pitch_modifier e;
	e.deserialize(st);
	CHECK(e.serialize()["formant_shift"].asFloat() == 2.0f && e.serialize()["algorithm"].asString() == "soundtouch", "kept with the soundtouch algorithm");
	Json::Value vm;
	vm["formant_shift"] = "not a number";
	Velocity_modifier vel;
	vel.deserialize(vm);
	CHECK(!vel.serialize().isMember("formant_shift"), "Velocity_modifier has no such key");
}

static bool dump(const char* path, const std::vector<float>& v)
{
	FILE* f = std::fopen(path, "wb");
	if (!f) return false;
	const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
	return std::fclose(f) == 0 && ok;
}

static void test_gpu(float semis, float shift, const char* in_path, const char* out_path)
{
	const int S = 60000, N = 1024;
	std::vector<float> x((size_t)S * 2, 0.0f);
	uint64_t st = 4242;
	for (size_t i = 0; i < x.size(); i++)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		x[i] = 0.5f * (float)((double)(st >> 40) / (double)(1ull << 24) - 0.5);
	}
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto pitch = std::make_shared<Pitch_modifier>();
	Json::Value v;
	v["pitch"] = (double)semis;
	v["formant_shift"] = (double)shift;
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(" << semis << ", formant_shift " << shift << ") -> sink runs: " << r.get_processor_resources().at(2)->error_text);
	if (!ok) return;
	std::vector<float> got;
	for (auto& f : sink->frames)
	{
		const Frame_data* d = f->data();
		CHECK(d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == 2, "interleaved stereo f32 out");
		const float* p = reinterpret_cast<const float*>(d->data[0]);
		got.insert(got.end(), p, p + (size_t)d->nb_samples * 2);
	}
	const float pf = std::pow(2.0f, semis / 12.0f);               // what Pitch_modifier passes
	const double phi = std::pow(2.0, (double)shift / 12.0);
	const int q = nae_stretch_formant_lifter(48000, N);
	nae_stretch_plan pl;
	CHECK(nae_stretch_plan_make_shift(1.0, (double)pf, phi, q, N, S, &pl) == 0, "plan");
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, pl.out_len * 2 * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig si{d_x, (size_t)S * 2, 1, 2}, so{d_o, pl.out_len * 2, 1, 2};
	std::vector<float> ref(pl.out_len * 2), plain(pl.out_len * 2);
	CHECK(nae_stretch_block_formant_shift_f32(ctx, 1.0, (double)pf, 0u, N, q, phi, &si, S, 2, 1, &so) == 0, "block call with the shift");
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, 0u, N, &si, S, 2, 1, &so) == 0, "block_n");
	CHECK(nae_memcpy_d2h(ctx, plain.data(), d_o, plain.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to the block call with the shift");
	CHECK(got.size() == plain.size() && std::memcmp(got.data(), plain.data(), ref.size() * sizeof(float)) != 0, "and not the call without it");
	CHECK(dump(in_path, x) && dump(out_path, got), "input and output written");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "json") test_json();
	else if (mode == "gpu" && argc == 6) test_gpu((float)std::atof(argv[2]), (float)std::atof(argv[3]), argv[4], argv[5]);
	else { std::cout << "usage: host_pv_fshift json | gpu <pitch> <shift> <in.f32> <out.f32>\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV FSHIFT OK " << mode << "\n";
	return 0;
}
