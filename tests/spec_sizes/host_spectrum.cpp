// host_spectrum.cpp — the host mirror's spectrum node at sizes other than 1024 (tests/test_spectrum_sizes_cpu.py builds it with the
// flags of tests/host/Makefile).  `json`: no GPU — the node's "fft_size" / "hop" keys round-trip, the defaults are not written,
// bad values are rejected.  `gpu`: a source -> spectrum(4096, 512) -> sink graph equals nae_spectrum_block_ex_f32 on the same
// samples bit for bit, with one frame per hop and pts advancing by hop / sample_rate.
#include "../node_harness.hpp"

// a rejected value leaves the node at its defaults
static bool rejects(const Json::Value& v, const std::string& field)
{
	Audio_spectrum node;
	return rejects(node, v, field) && node.fft_size == 1024 && node.hop == 256;
}

static void test_json()
{
	Audio_spectrum node;
	CHECK(node.fft_size == 1024 && node.hop == 256, "defaults 1024 / 256");
	CHECK(node.serialize().isNull(), "defaults are not written");
	node.deserialize(Json::Value());
	CHECK(node.fft_size == 1024 && node.hop == 256 && node.serialize().isNull(), "a project without the keys keeps the defaults");
	for (int n : {256, 512, 1024, 2048, 4096})
		for (int h : {1, 7, n / 4, n})
		{
			Json::Value v;
			v["fft_size"] = n;
			v["hop"] = h;
			Audio_spectrum a, b;
			a.deserialize(v);
			CHECK(a.fft_size == n && a.hop == h, "read " << n << " / " << h);
			const Json::Value w = a.serialize();
			CHECK(w.isMember("fft_size") == (n != 1024) && w.isMember("hop") == (h != 256), "only non-defaults written: " << n << " / " << h);
			b.deserialize(w);
			CHECK(b.fft_size == n && b.hop == h, "round trip " << n << " / " << h);
		}
	{
		Json::Value v;
		v["hop"] = 512;
		Audio_spectrum a;
		a.deserialize(v);
		CHECK(a.fft_size == 1024 && a.hop == 512 && !a.serialize().isMember("fft_size"), "hop alone");
	}
	for (int n : {0, 128, 1000, 8192, -1024})
	{
		Json::Value v;
		v["fft_size"] = n;
		CHECK(rejects(v, "fft_size"), "fft_size " << n << " rejected");
	}
	{
		Json::Value v;
		v["fft_size"] = 1024.5;
		CHECK(rejects(v, "fft_size"), "fractional fft_size rejected");
		Json::Value s;
		s["fft_size"] = "big";
		CHECK(rejects(s, "fft_size"), "string fft_size rejected");
	}
	for (int h : {0, -1, 1025})
	{
		Json::Value v;
		v["hop"] = h;
		CHECK(rejects(v, "hop"), "hop " << h << " rejected at 1024");
	}
	{
		Json::Value v;
		v["fft_size"] = 256;
		CHECK(rejects(v, "hop") == false, "256 with the default hop 256 is valid");
		v["hop"] = 257;
		CHECK(rejects(v, "hop"), "hop 257 rejected at 256");
	}
}

static void test_gpu()
{
	const int n_fft = 4096, hop = 512, S = 40000, bins = n_fft / 2 + 1;
	std::vector<float> x((size_t)S * 2);
	uint64_t st = 12345;
	for (auto& v : x)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		v = (float)((double)(st >> 40) / (double)(1ull << 24) * 2.0 - 1.0);
	}
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto spec = std::make_shared<Audio_spectrum>();
	Json::Value v;
	v["fft_size"] = n_fft;
	v["hop"] = hop;
	spec->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, spec); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> spectrum(4096, 512) -> sink runs: " << r.get_processor_resources().at(2)->error_text);
	if (!ok) return;
	const size_t F = nae_spectrum_frames_ex(S, n_fft, hop);
	CHECK(F == (size_t)(S - n_fft) / hop + 1, "frames_ex");
	// the block call on the same samples, through a context of its own
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, F * 2 * bins * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig sig{d_x, (size_t)S * 2, 1, 2};
	CHECK(nae_spectrum_block_ex_f32(ctx, n_fft, hop, &sig, S, 2, 1, static_cast<float*>(d_o), F * 2 * bins) == 0, "block_ex");
	std::vector<float> ref(F * 2 * bins);
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(sink->frames.size() == F, "one output frame per hop: " << sink->frames.size() << " vs " << F);
	bool same = sink->frames.size() == F, pts_ok = same;
	for (size_t f = 0; f < sink->frames.size() && same; f++)
	{
		const Frame_data* d = sink->frames[f]->data();
		same = d->nb_samples == bins && d->format == AV_SAMPLE_FMT_FLTP && d->ch_layout.nb_channels == 2;
		for (int c = 0; c < 2 && same; c++) same = std::memcmp(d->data[c], &ref[(f * 2 + c) * bins], bins * sizeof(float)) == 0;
		double t = 500000 * (1 / 1000000.0);   // the first input frame's pts in seconds, as the node reads it
		for (size_t i = 0; i < f; i++) t += (double)hop / 48000;
		pts_ok = pts_ok && d->pts == (int64_t)(t * 1000000) && d->time_base.num == 1 && d->time_base.den == 1000000;
	}
	CHECK(same, "graph frames bit-identical to nae_spectrum_block_ex_f32");
	CHECK(pts_ok, "pts = start + f * hop / sample_rate");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "json";
	if (mode == "json") test_json();
	else if (mode == "gpu") test_gpu();
	else { std::cout << "usage: host_spectrum json|gpu\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST SPECTRUM OK " << mode << "\n";
	return 0;
}
