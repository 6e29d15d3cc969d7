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

static void test_registry() { check_registry("audio_filter"); }

static void test_gpu()
{
	const int S = 20000, L = 513, D = (L - 1) / 2, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	Json::Value v;
	v["kind"] = "lowpass";
	v["f_hi"] = 1000;
	v["taps"] = L;
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_filter>(x, v, frame_size, sink, &error);
	CHECK(ok, "source -> audio_filter -> sink runs: " << error);
	if (!ok) return;
	// the block call on the same samples, and on the samples extended by L - 1 zeros (the flushed tail)
	std::vector<float> taps(L);
	CHECK(nae_fir_design(0, 48000, 0, 1000, L, taps.data()) == 0, "design");
	const size_t E = (size_t)S + L - 1;
	std::vector<float> xe(E * 2, 0.0f);
	std::memcpy(xe.data(), x.data(), x.size() * sizeof(float));
	const auto fir = [&](size_t n) { return [&taps, n](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_fir_block_f32(ctx, taps.data(), L, 0, sx, n, 2, 1, sy); }; };
	const std::vector<float> y = block_call(x, S, fir(S)), ye = block_call(xe, E, fir(E));
	if (y.empty() || ye.empty()) return;
	// sample n = y[n + D] inside the input, past its end the zero-extended call's
	std::vector<float> want((size_t)S * 2);
	for (size_t n = 0; n < (size_t)S; n++)
		for (int c = 0; c < 2; c++) want[n * 2 + c] = n + D < (size_t)S ? y[(n + D) * 2 + c] : ye[(n + D) * 2 + c];
	check_frames(*sink, want, S, frame_size, "sample n = y[n + 256] of the block call, past the input's end the flushed tail");
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "FIR", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
