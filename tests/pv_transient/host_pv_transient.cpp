// host_pv_transient.cpp — the host mirror's "transients" key on Velocity_modifier and Pitch_modifier (tests/test_pv_transient_cpu.py,
// tests/test_gpu_pv_transient.py).  Built by its tests with tests/node_harness.py.
//
// `json`: no GPU — absent means false and is not written; true round-trips; false is not written; a value that is not a bool is "Wrong field:
// transients"; it combines with "phase_lock", "fft_size" and (Pitch_modifier) "formant"; with "algorithm": "soundtouch" it is kept, with
// "phase_lock" too.
// `gpu`: source -> Pitch_modifier {"pitch": 3, "fft_size": 2048, "transients": true} -> sink through the fiber runner equals the block call
// nae_stretch_block_n_f32(2048, NAE_STRETCH_TRANSIENTS) on the same samples bit for bit, and differs from the unflagged call (the input is a
// click train, which has onsets).  `gpu_lock`: the same with {"pitch": 3, "phase_lock": true, "transients": true} against
// nae_stretch_block_n_f32(1024, NAE_STRETCH_PHASE_LOCK | NAE_STRETCH_TRANSIENTS) and the locked call without the flag.
#include "../node_harness.hpp"

template <class Node>
static void json_transients(const char* name, bool pitch_node)
{
	Node node;
	CHECK(!node.serialize().isMember("transients"), name << ": a default node writes no transients");
	Json::Value on;
	on["transients"] = true;
	Node a;
	a.deserialize(on);
	const Json::Value w = a.serialize();
	CHECK(w.isMember("transients") && w["transients"].isBool() && w["transients"].asBool(), name << ": true is written back");
	Node b;
	b.deserialize(w);
	CHECK(b.serialize()["transients"].isBool() && b.serialize()["transients"].asBool(), name << ": round trip");
	Node d;
	d.deserialize(on);
	d.deserialize(Json::Value());
	CHECK(!d.serialize().isMember("transients"), name << ": a missing key means false");
	Json::Value off;
	off["transients"] = false;
	Node c;
	c.deserialize(off);
	CHECK(!c.serialize().isMember("transients"), name << ": false is not written");
	for (const Json::Value& bad : {Json::Value(1), Json::Value(0), Json::Value("true"), Json::Value(1.5)})
	{
		Json::Value v;
		v["transients"] = bad;
		CHECK(rejects<Node>(v, "transients"), name << ": a non-bool transients is rejected");
	}
	Json::Value lk;
	lk["transients"] = true;
	lk["phase_lock"] = true;
	Node e;
	e.deserialize(lk);
	CHECK(e.serialize()["phase_lock"].asBool() && e.serialize()["transients"].asBool() && !e.serialize().isMember("fft_size"),
		  name << ": combines with phase_lock");
	Json::Value lk2048 = lk;
	lk2048["fft_size"] = 2048;
	CHECK(rejects<Node>(lk2048, "fft_size"), name << ": phase_lock with 2048 is still rejected by fft_size");
	Json::Value sz;
	sz["transients"] = true;
	sz["fft_size"] = 4096;
	if (pitch_node) sz["formant"] = true;
	Node f;
	f.deserialize(sz);
	const Json::Value fw = f.serialize();
	CHECK(fw["transients"].asBool() && fw["fft_size"].asInt() == 4096, name << ": combines with fft_size");
	if (pitch_node) CHECK(fw["formant"].asBool(), name << ": combines with formant");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["transients"] = true;
	Node g;
	g.deserialize(st);
	CHECK(g.serialize()["transients"].asBool() && g.serialize()["algorithm"].asString() == "soundtouch", name << ": kept with the soundtouch algorithm");
	st["phase_lock"] = true;
	Node h;
	h.deserialize(st);
	CHECK(h.serialize()["transients"].asBool() && h.serialize()["phase_lock"].asBool(), name << ": both kept with the soundtouch algorithm");
}

static void test_gpu(bool lock)
{
	const int S = 60000, N = lock ? 1024 : 2048;
	const unsigned base = lock ? NAE_STRETCH_PHASE_LOCK : 0u;
	const float semis = 3.0f;
	std::vector<float> x((size_t)S * 2, 0.0f);
	uint64_t st = 777;
	for (size_t i = 0; i < x.size(); i++)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		x[i] = 0.02f * (float)((double)(st >> 40) / (double)(1ull << 24) - 0.5);
	}
	for (int p = 3000; p < S; p += 9000) x[(size_t)p * 2] = x[(size_t)p * 2 + 1] = 0.9f;   // clicks over quiet noise
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto pitch = std::make_shared<Pitch_modifier>();
	Json::Value v;
	v["pitch"] = (double)semis;
	if (lock) v["phase_lock"] = true;
	else v["fft_size"] = N;
	v["transients"] = true;
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(+3, " << (lock ? "phase_lock" : "fft_size 2048") << ", transients) -> sink runs: " << r.get_processor_resources().at(2)->error_text);
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
	CHECK(nae_stretch_plan_make_n(1.0, (double)pf, N, S, &pl) == 0, "plan");
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, pl.out_len * 2 * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig si{d_x, (size_t)S * 2, 1, 2}, so{d_o, pl.out_len * 2, 1, 2};
	std::vector<float> ref(pl.out_len * 2), plain(pl.out_len * 2);
	CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, base | NAE_STRETCH_TRANSIENTS, N, &si, S, 2, 1, &so) == 0, "block_n with transients");
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, base, N, &si, S, 2, 1, &so) == 0, "block_n");
	CHECK(nae_memcpy_d2h(ctx, plain.data(), d_o, plain.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to the flagged block call");
	CHECK(got.size() == plain.size() && std::memcmp(got.data(), plain.data(), ref.size() * sizeof(float)) != 0, "and not the unflagged one");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "json") { json_transients<Velocity_modifier>("Velocity_modifier", false); json_transients<Pitch_modifier>("Pitch_modifier", true); }
	else if (mode == "gpu") test_gpu(false);
	else if (mode == "gpu_lock") test_gpu(true);
	else { std::cout << "usage: host_pv_transient json|gpu|gpu_lock\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV TRANSIENT OK " << mode << "\n";
	return 0;
}
