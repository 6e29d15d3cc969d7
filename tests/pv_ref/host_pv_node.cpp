// host_pv_node.cpp — the host mirror's vocoder keys on Velocity_modifier and Pitch_modifier: "fft_size" (tests/test_pv_sizes_cpu.py,
// tests/test_gpu_pv_sizes.py), "phase_lock" (tests/test_pv_lock_cpu.py, tests/test_gpu_pv_lock.py) and "formant", Pitch_modifier only
// (tests/test_pv_formant_cpu.py, tests/test_gpu_pv_formant.py).  Built by its tests with the flags of tests/host/Makefile.
//
// `json <key>`: no GPU — the key round-trips and is not written at its default.  fft_size: a value that is not 512 / 1024 / 2048 / 4096, or
// a size other than 1024 with "phase_lock": true, is "Wrong field: fft_size"; phase_lock: a non-bool is "Wrong field: phase_lock"; formant:
// a non-bool is "Wrong field: formant", it combines with phase_lock and fft_size, and Velocity_modifier has no such key.
// `gpu <key> [out.f32]`: source -> Pitch_modifier {"pitch": 3, "fft_size": 4096} / {"pitch": 3, "phase_lock": true} / {"pitch": 4,
// "formant": true} -> sink through the fiber runner equals the block call nae_stretch_block_n_f32(4096) / nae_stretch_block_ex_f32
// (NAE_STRETCH_PHASE_LOCK, and differs from the unlocked call) / nae_stretch_block_formant_f32 with the node's lifter on the same samples
// bit for bit; the input and the graph's output are written to out.f32 for the test to compare with the CPU statement.
#include "../node_harness.hpp"

template <class Node>
static void json_fft_size(const char* name)
{
	Node node;
	CHECK(!node.serialize().isMember("fft_size"), name << ": a default node writes no fft_size");
	for (int n : {512, 2048, 4096})
	{
		Json::Value v;
		v["fft_size"] = n;
		Node a;
		a.deserialize(v);
		const Json::Value w = a.serialize();
		CHECK(w.isMember("fft_size") && w["fft_size"].asInt() == n, name << ": " << n << " is written back");
		Node b;
		b.deserialize(w);
		CHECK(b.serialize()["fft_size"].asInt() == n, name << ": round trip " << n);
		Node d;
		d.deserialize(v);
		d.deserialize(Json::Value());
		CHECK(!d.serialize().isMember("fft_size"), name << ": a missing key means 1024");
	}
	Json::Value k1024;
	k1024["fft_size"] = 1024;
	Node c;
	c.deserialize(k1024);
	CHECK(!c.serialize().isMember("fft_size"), name << ": 1024 is not written");
	for (const Json::Value& bad : {Json::Value(256), Json::Value(8192), Json::Value(1000), Json::Value(2048.5), Json::Value(1e12), Json::Value(-1e12), Json::Value("2048"), Json::Value(true)})
	{
		Json::Value v;
		v["fft_size"] = bad;
		CHECK(rejects<Node>(v, "fft_size"), name << ": bad fft_size rejected");
	}
	Json::Value lk;
	lk["fft_size"] = 2048;
	lk["phase_lock"] = true;
	CHECK(rejects<Node>(lk, "fft_size"), name << ": phase_lock with 2048 rejected");
	lk["fft_size"] = 1024;
	Node e;
	e.deserialize(lk);
	CHECK(e.serialize()["phase_lock"].asBool() && !e.serialize().isMember("fft_size"), name << ": phase_lock with 1024 accepted");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["fft_size"] = 4096;
	Node f;
	f.deserialize(st);
	CHECK(f.serialize()["fft_size"].asInt() == 4096 && f.serialize()["algorithm"].asString() == "soundtouch", name << ": kept with the soundtouch algorithm");
}

template <class Node>
static void json_phase_lock(const char* name)
{
	Node node;
	CHECK(!node.serialize().isMember("phase_lock"), name << ": a default node writes no phase_lock");
	Json::Value on;
	on["phase_lock"] = true;
	Node a;
	a.deserialize(on);
	const Json::Value w = a.serialize();
	CHECK(w.isMember("phase_lock") && w["phase_lock"].isBool() && w["phase_lock"].asBool(), name << ": true is written back");
	Node b;
	b.deserialize(w);
	CHECK(b.serialize()["phase_lock"].isBool() && b.serialize()["phase_lock"].asBool(), name << ": round trip");
	Json::Value off;
	off["phase_lock"] = false;
	Node c;
	c.deserialize(off);
	CHECK(!c.serialize().isMember("phase_lock"), name << ": false is not written");
	Node d;
	d.deserialize(on);
	d.deserialize(Json::Value());
	CHECK(!d.serialize().isMember("phase_lock"), name << ": a missing key means false");
	for (const Json::Value& bad : {Json::Value(1), Json::Value(0.5), Json::Value("true")})
	{
		Json::Value v;
		v["phase_lock"] = bad;
		CHECK(rejects<Node>(v, "phase_lock"), name << ": non-bool phase_lock rejected");
	}
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["phase_lock"] = true;
	Node e;
	e.deserialize(st);
	CHECK(e.serialize()["phase_lock"].asBool() && e.serialize()["algorithm"].asString() == "soundtouch", name << ": kept with the soundtouch algorithm");
}

static void json_formant()
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
		CHECK(rejects<Pitch_modifier>(x, "formant"), "a formant that is not a bool is rejected");
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

static void test_gpu(const std::string& key, const char* out_path)
{
	const bool sizes = key == "fft_size", lock = key == "phase_lock";
	const int S = 60000, N = sizes ? 4096 : 1024;
	const float semis = key == "formant" ? 4.0f : 3.0f;
	const char* label = sizes ? "+3, fft_size 4096" : lock ? "+3, phase_lock" : "+4, formant";
	const char* call = sizes ? "the 4096-point block call" : lock ? "the locked block call" : "the formant block call";
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
	v[key] = sizes ? Json::Value(N) : Json::Value(true);
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(" << label << ") -> sink runs: " << r.get_processor_resources().at(2)->error_text);
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
	nae_stretch_plan pl;
	CHECK((lock ? nae_stretch_plan_make(1.0, (double)pf, S, &pl) : nae_stretch_plan_make_n(1.0, (double)pf, N, S, &pl)) == 0, "plan");
	const int lifter = nae_stretch_formant_lifter(48000, N);
	if (key == "formant") CHECK(lifter == 68, "lifter at 48 kHz: " << lifter);
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, pl.out_len * 2 * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig si{d_x, (size_t)S * 2, 1, 2}, so{d_o, pl.out_len * 2, 1, 2};
	if (sizes) CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, 0u, N, &si, S, 2, 1, &so) == 0, "block_n");
	else if (lock) CHECK(nae_stretch_block_ex_f32(ctx, 1.0, (double)pf, NAE_STRETCH_PHASE_LOCK, &si, S, 2, 1, &so) == 0, "block_ex");
	else CHECK(nae_stretch_block_formant_f32(ctx, 1.0, (double)pf, 0u, N, lifter, &si, S, 2, 1, &so) == 0, "block_formant");
	std::vector<float> ref(pl.out_len * 2), unlocked(pl.out_len * 2);
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	if (lock)
	{
		CHECK(nae_stretch_block_f32(ctx, 1.0, (double)pf, &si, S, 2, 1, &so) == 0, "block");
		CHECK(nae_memcpy_d2h(ctx, unlocked.data(), d_o, unlocked.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	}
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to " << call);
	if (lock)
		CHECK(got.size() == unlocked.size() && std::memcmp(got.data(), unlocked.data(), ref.size() * sizeof(float)) != 0, "and not the unlocked one");
	if (!out_path) return;
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
	const std::string mode = argc > 1 ? argv[1] : "", key = argc > 2 ? argv[2] : "";
	const bool key_ok = key == "fft_size" || key == "phase_lock" || key == "formant";
	if (mode == "json" && key == "fft_size") { json_fft_size<Velocity_modifier>("Velocity_modifier"); json_fft_size<Pitch_modifier>("Pitch_modifier"); }
	else if (mode == "json" && key == "phase_lock") { json_phase_lock<Velocity_modifier>("Velocity_modifier"); json_phase_lock<Pitch_modifier>("Pitch_modifier"); }
	else if (mode == "json" && key == "formant") json_formant();
	else if (mode == "gpu" && key_ok) test_gpu(key, argc > 3 ? argv[3] : nullptr);
	else { std::cout << "usage: host_pv_node json|gpu fft_size|phase_lock|formant [out.f32]\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV NODE OK " << mode << " " << key << "\n";
	return 0;
}
