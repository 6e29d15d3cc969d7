// host_fir_node.cpp — the host mirror's filter node (tests/test_fir_cpu.py and tests/test_gpu_fir.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_filter round-trips, the defaults are not written back, wrong values are rejected.  `registry`: no GPU —
// the processor map after register_all_processors() and after register_extension_processors().  `gpu`: a source -> audio_filter -> sink
// graph delivers the frames it received, with their sizes and pts, and sample n equals y[n + (L - 1) / 2] of nae_fir_block_f32 bit for bit.
#include "../node_harness.hpp"
#include "processor/audio-filter.hpp"

using Kind = Audio_filter::Kind;

static bool at_defaults(const Audio_filter& n)
{
	return n.kind == Kind::Lowpass && n.f_lo == 100 && n.f_hi == 1000 && n.taps == 513 && n.fft_size == 0;
}

// a rejected value leaves the node at its defaults
static bool rejects(const Json::Value& v, const std::string& field)
{
	Audio_filter node;
	return rejects(node, v, field) && at_defaults(node);
}

static void test_json()
{
	Audio_filter node;
	CHECK(at_defaults(node), "defaults lowpass / 100 / 1000 / 513 / pick");
	CHECK(node.serialize().isNull(), "defaults are not written");
	node.deserialize(Json::Value());
	CHECK(at_defaults(node) && node.serialize().isNull(), "a project without the keys keeps the defaults");
	const char* kinds[] = {"lowpass", "highpass", "bandpass", "bandstop"};
	for (int k = 0; k < 4; k++)
		for (int taps : {1, 65, 513, 2049})
			for (int fft : {0, 4096})
			{
				Json::Value v;
				v["kind"] = kinds[k];
				v["f_lo"] = 250.5;
				v["f_hi"] = 4000;
				v["taps"] = taps;
				if (fft) v["fft_size"] = fft;
				Audio_filter a, b;
				a.deserialize(v);
				CHECK((int)a.kind == k && a.f_lo == 250.5f && a.f_hi == 4000 && a.taps == taps && a.fft_size == fft, "read " << kinds[k] << " / " << taps << " / " << fft);
				const Json::Value w = a.serialize();
				CHECK(w.isMember("kind") == (k != 0) && w.isMember("f_lo") && w.isMember("f_hi") && w.isMember("taps") == (taps != 513) &&
						  w.isMember("fft_size") == (fft != 0),
					  "only non-defaults written: " << kinds[k] << " / " << taps << " / " << fft);
				b.deserialize(w);
				CHECK(b.kind == a.kind && b.f_lo == a.f_lo && b.f_hi == a.f_hi && b.taps == a.taps && b.fft_size == a.fft_size, "round trip");
			}
	{
		Json::Value v;
		v["fft_size"] = 1024;   // the pick for 513 taps, given explicitly: kept and written back
		Audio_filter a;
		a.deserialize(v);
		CHECK(a.fft_size == 1024 && a.serialize().isMember("fft_size") && a.serialize()["fft_size"].asInt() == 1024, "fft_size written back when present");
	}
	{
		Json::Value s;
		s["taps"] = "many";
		CHECK(rejects(s, "taps"), "string taps rejected");
	}
	for (double t : {0.0, -1.0, 2.0, 512.0, 2051.0, 513.5, 1e12})
	{
		Json::Value v;
		v["taps"] = t;
		CHECK(rejects(v, "taps"), "taps " << t << " rejected");
	}
	for (const char* key : {"f_lo", "f_hi"})
	{
		Json::Value s, z, n;
		s[key] = "low";
		z[key] = 0;
		n[key] = -20.0;
		CHECK(rejects(s, key) && rejects(z, key) && rejects(n, key), key << ": a string, zero and a negative value rejected");
	}
	{
		Json::Value s, u;
		s["kind"] = 1;
		u["kind"] = "notch";
		CHECK(rejects(s, "kind") && rejects(u, "kind"), "kind: a number and an unknown name rejected");
	}
	for (double n : {0.0, 256.0, 1000.0, 8192.0, 1024.5, -1024.0})
	{
		Json::Value v;
		v["fft_size"] = n;
		CHECK(rejects(v, "fft_size"), "fft_size " << n << " rejected");
	}
	{
		Json::Value v, s;
		v["fft_size"] = 512;    // 513 taps need 1024
		s["fft_size"] = "big";
		CHECK(rejects(v, "fft_size") && rejects(s, "fft_size"), "fft_size too small for the taps, and a string, rejected");
		v["taps"] = 257;
		CHECK(!rejects(v, "fft_size"), "257 taps fit 512");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_filter a;
		a.taps = 600;
		a.fft_size = 512;
		a.kind = Kind::Bandpass;
		a.f_lo = 900;
		a.f_hi = 300;
		CHECK(a.draw_content(false) == false && a.taps == 601 && a.fft_size == 0 && a.f_lo == 300 && a.f_hi == 900, "draw_content: odd taps, pick, corners in order");
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
	print_registry();
	CHECK(infra::Processor::processor_map.size() == 7 && infra::Processor::processor_map.count("audio_filter") == 0, "the reference's list: 7 entries");
	infra::register_extension_processors();
	print_registry();
	CHECK(infra::Processor::processor_map.size() == 8 && infra::Processor::processor_map.count("audio_filter") == 1, "with the extensions: 8 entries");
	if (infra::Processor::processor_map.count("audio_filter"))
	{
		const auto node = infra::Processor::processor_map.at("audio_filter").generate();
		const auto pins = node->get_pin_attributes();
		CHECK(node->get_processor_info_non_static().identifier == "audio_filter" && pins.size() == 2, "generate() gives the node: two pins");
		int inputs = 0;
		for (const auto& p : pins) inputs += p.is_input && p.type.get() == typeid(Audio_stream);
		CHECK(inputs == 1, "one audio input pin, one audio output pin");
	}
}

static void test_gpu()
{
	const int S = 20000, L = 513, D = (L - 1) / 2, frame_size = 1152;
	std::vector<float> x((size_t)S * 2);
	uint64_t st = 4711;
	for (auto& v : x)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		v = (float)((double)(st >> 40) / (double)(1ull << 24) * 2.0 - 1.0);
	}
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	src->frame_size = frame_size;
	auto filter = std::make_shared<Audio_filter>();
	Json::Value v;
	v["kind"] = "lowpass";
	v["f_hi"] = 1000;
	v["taps"] = L;
	filter->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, filter); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> audio_filter -> sink runs: " << r.get_processor_resources().at(2)->error_text);
	if (!ok) return;
	// the block call on the same samples, and on the samples extended by L - 1 zeros (the flushed tail), through a context of its own
	std::vector<float> taps(L);
	CHECK(nae_fir_design(0, 48000, 0, 1000, L, taps.data()) == 0, "design");
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return;
	const size_t E = (size_t)S + L - 1;
	std::vector<float> xe(E * 2, 0.0f), y((size_t)S * 2), ye(E * 2);
	std::memcpy(xe.data(), x.data(), x.size() * sizeof(float));
	void *d_x = nullptr, *d_y = nullptr;
	CHECK(nae_malloc(ctx, xe.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, ye.size() * sizeof(float), &d_y) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, xe.data(), xe.size() * sizeof(float)) == 0, "h2d");
	const nae_sig sx{d_x, 0, 1, 2}, sy{d_y, 0, 1, 2};
	CHECK(nae_fir_block_f32(ctx, taps.data(), L, 0, &sx, S, 2, 1, &sy) == 0, "block call");
	CHECK(nae_memcpy_d2h(ctx, y.data(), d_y, y.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	CHECK(nae_fir_block_f32(ctx, taps.data(), L, 0, &sx, E, 2, 1, &sy) == 0, "block call on the zero-extended input");
	CHECK(nae_memcpy_d2h(ctx, ye.data(), d_y, ye.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	nae_free(ctx, d_x);
	nae_free(ctx, d_y);
	nae_ctx_destroy(ctx);

	const size_t n_frames = ((size_t)S + frame_size - 1) / frame_size;
	CHECK(sink->frames.size() == n_frames, "as many frames as the source sent: " << sink->frames.size() << " vs " << n_frames);
	size_t pos = 0, bad = 0;
	bool shape_ok = true;
	for (size_t f = 0; f < sink->frames.size(); f++)
	{
		const Frame_data* d = sink->frames[f]->data();
		const int want_n = (int)std::min<size_t>(frame_size, (size_t)S - std::min<size_t>(S, f * frame_size));
		const int64_t want_pts = (int64_t)((0.5 + double(f * frame_size) / 48000) * 1000000);   // the source's own formula
		shape_ok = shape_ok && d->nb_samples == want_n && d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == 2 && d->sample_rate == 48000 &&
				   d->pts == want_pts && d->time_base.num == 1 && d->time_base.den == 1000000;
		const float* got = reinterpret_cast<const float*>(d->data[0]);
		for (int i = 0; i < d->nb_samples && pos < (size_t)S; i++, pos++)
			for (int c = 0; c < 2; c++)
			{
				const size_t n = pos + D;
				const float want = n < (size_t)S ? y[n * 2 + c] : ye[n * 2 + c];
				bad += std::memcmp(&got[i * 2 + c], &want, sizeof(float)) != 0;
			}
	}
	CHECK(shape_ok, "frames of the input's sizes, format FLT, the source's pts and time base");
	CHECK(pos == (size_t)S, "as many samples as the source sent: " << pos);
	CHECK(bad == 0, "sample n = y[n + 256] of the block call, past the input's end the flushed tail: " << bad << " words differ");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "json";
	if (mode == "json") test_json();
	else if (mode == "registry") test_registry();
	else if (mode == "gpu") test_gpu();
	else { std::cout << "usage: host_fir_node json|registry|gpu\n"; return 2; }
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST FIR OK " << mode << "\n";
	return 0;
}
