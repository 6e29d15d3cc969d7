// host_pv_link.cpp — the host mirror's "link_channels" key on Velocity_modifier and Pitch_modifier (tests/test_pv_link_cpu.py,
// tests/test_gpu_pv_link.py).  Built by its tests with tests/node_harness.py.
//
// `json`: no GPU — absent means false and is not written (the default serialisation is unchanged); true round-trips; false is not written; a
// value that is not a bool is "Wrong field: link_channels"; it combines with "phase_lock", "fft_size", "transients" and (Pitch_modifier)
// "formant" and "formant_shift"; with "algorithm": "soundtouch" it is kept.
// `gpu`: source -> Pitch_modifier {"pitch": 3, "fft_size": 2048, "transients": true, "link_channels": true} -> sink through the fiber runner
// equals the block call nae_stretch_block_n_f32(2048, NAE_STRETCH_TRANSIENTS | NAE_STRETCH_LINK_CHANNELS) on the same samples bit for bit, and
// differs from the call without the link (the input has clicks in the left channel only).  `gpu_lock`: the same with {"pitch": 3,
// "phase_lock": true, "link_channels": true} against nae_stretch_block_n_f32(1024, NAE_STRETCH_PHASE_LOCK | NAE_STRETCH_LINK_CHANNELS).
#include "../node_harness.hpp"

template <class Node>
static void json_link(const char* name, bool pitch_node)
{
	Node node;
	const Json::Value dflt = node.serialize();
	CHECK(!dflt.isMember("link_channels"), name << ": a default node writes no link_channels");
	CHECK(dflt.size() == (pitch_node ? 1u : 2u), name << ": the default serialisation keeps its key set");
	Json::Value on;
	on["link_channels"] = true;
	Node a;
	a.deserialize(on);
	const Json::Value w = a.serialize();
	CHECK(w.isMember("link_channels") && w["link_channels"].isBool() && w["link_channels"].asBool(), name << ": true is written back");
	Node b;
	b.deserialize(w);
	CHECK(b.serialize()["link_channels"].isBool() && b.serialize()["link_channels"].asBool(), name << ": round trip");
	Node d;
	d.deserialize(on);
	d.deserialize(Json::Value());
	CHECK(!d.serialize().isMember("link_channels"), name << ": a missing key means false");
	Json::Value off;
	off["link_channels"] = false;
	Node c;
	c.deserialize(off);
	CHECK(!c.serialize().isMember("link_channels"), name << ": false is not written");
	for (const Json::Value& bad : {Json::Value(1), Json::Value(0), Json::Value("true"), Json::Value(1.5)})
	{
		Json::Value v;
		v["link_channels"] = bad;
		CHECK(rejects<Node>(v, "link_channels"), name << ": a non-bool link_channels is rejected");
	}
	Json::Value lk;
	lk["link_channels"] = true;
	lk["phase_lock"] = true;
	lk["transients"] = true;
	Node e;
	e.deserialize(lk);
	const Json::Value ew = e.serialize();
	CHECK(ew["phase_lock"].asBool() && ew["transients"].asBool() && ew["link_channels"].asBool() && !ew.isMember("fft_size"),
		  name << ": combines with phase_lock and transients");
	Json::Value sz;
	sz["link_channels"] = true;
	sz["transients"] = true;
	sz["fft_size"] = 4096;
	if (pitch_node) { sz["formant"] = true; sz["formant_shift"] = 2.0; }
	Node f;
	f.deserialize(sz);
	const Json::Value fw = f.serialize();
	CHECK(fw["link_channels"].asBool() && fw["transients"].asBool() && fw["fft_size"].asInt() == 4096, name << ": combines with fft_size");
	if (pitch_node) CHECK(fw["formant"].asBool() && fw["formant_shift"].asDouble() == 2.0, name << ": combines with formant and formant_shift");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["link_channels"] = true;
	Node g;
	g.deserialize(st);
	CHECK(g.serialize()["link_channels"].asBool() && g.serialize()["algorithm"].asString() == "soundtouch", name << ": kept with the soundtouch algorithm");
}

static void test_gpu(bool lock)
{
	const int S = 60000, N = lock ? 1024 : 2048;
	const unsigned base = lock ? NAE_STRETCH_PHASE_LOCK : NAE_STRETCH_TRANSIENTS;
	const float semis = 3.0f;
	std::vector<float> x((size_t)S * 2, 0.0f);
	uint64_t st = 777;
	for (size_t i = 0; i < x.size(); i++)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		x[i] = 0.02f * (float)((double)(st >> 40) / (double)(1ull << 24) - 0.5);
	}
	for (int p = 3000; p < S; p += 9000) x[(size_t)p * 2] = 0.9f;   // clicks in the left channel only, over quiet independent noise
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto pitch = std::make_shared<Pitch_modifier>();
	Json::Value v;
	v["pitch"] = (double)semis;
	if (lock) v["phase_lock"] = true;
	else { v["fft_size"] = N; v["transients"] = true; }
	v["link_channels"] = true;
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(+3, " << (lock ? "phase_lock" : "fft_size 2048, transients") << ", link_channels) -> sink runs: "
								  << r.get_processor_resources().at(2)->error_text);
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
	CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, base | NAE_STRETCH_LINK_CHANNELS, N, &si, S, 2, 1, &so) == 0, "block_n with the link");
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	CHECK(nae_stretch_block_n_f32(ctx, 1.0, (double)pf, base, N, &si, S, 2, 1, &so) == 0, "block_n");
	CHECK(nae_memcpy_d2h(ctx, plain.data(), d_o, plain.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to the linked block call");
	CHECK(got.size() == plain.size() && std::memcmp(got.data(), plain.data(), ref.size() * sizeof(float)) != 0, "and not the unlinked one");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "json") { json_link<Velocity_modifier>("Velocity_modifier", false); json_link<Pitch_modifier>("Pitch_modifier", true); }
	else if (mode == "gpu") test_gpu(false);
	else if (mode == "gpu_lock") test_gpu(true);
	else { std::cout << "usage: host_pv_link json|gpu|gpu_lock\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV LINK OK " << mode << "\n";
	return 0;
}
