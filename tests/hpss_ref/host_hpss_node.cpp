// host_hpss_node.cpp — the host mirror's separation node (tests/test_hpss_cpu.py and tests/test_gpu_hpss.py build it through
// tests/node_harness.py).  `json`: no GPU — every key of audio_separation round-trips, the defaults are not written back, wrong values are
// rejected with their key.  `registry`: no GPU — the processor map after the thirteen existing registration calls, each with the count it had,
// and after register_separation_processors().  `gpu`: a source -> audio_separation -> sink graph delivers the frames it received, with their
// sizes and pts, and the samples of nae_hpss_block_f32 with the designed parameters, bit for bit; the defaults take the clicks out of a chord.
#include "../node_harness.hpp"
#include "processor/audio-separation.hpp"
#include "nae_dsp_spec.h"

static const char* real_keys[] = {"harmonic_db", "percussive_db"};
static const char* int_keys[] = {"time_span", "freq_span"};

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_separation node;
	node.deserialize(with("harmonic_db", -7.0));
	return rejects(node, v, field) && node.harmonic_db == -7 && node.percussive_db == -120 && node.fft_size == 2048 && node.time_span == 8 &&
		   node.mask == Audio_separation::Mask::Soft;
}

static void test_json()
{
	Audio_separation node;
	CHECK(node.harmonic_db == 0 && node.percussive_db == -120 && node.mask == Audio_separation::Mask::Soft && node.fft_size == 2048 && node.time_span == 8 &&
			  node.freq_span == 8,
		  "defaults: 0 dB, -120 dB, soft, 2048, 8 frames, 8 bins");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull() && node.fft_size == 2048, "a project without the keys keeps the defaults");
	{
		Json::Value v;
		v["harmonic_db"] = -120.0;
		v["percussive_db"] = 3.5;
		v["mask"] = "hard";
		v["fft_size"] = 512;
		v["time_span"] = 3;
		v["freq_span"] = 0;
		Audio_separation a, c;
		a.deserialize(v);
		const auto all = [](const Audio_separation& s) {
			return s.harmonic_db == -120 && s.percussive_db == 3.5 && s.mask == Audio_separation::Mask::Hard && s.fft_size == 512 && s.time_span == 3 && s.freq_span == 0;
		};
		CHECK(all(a), "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 6 && w["harmonic_db"].asDouble() == -120 && w["percussive_db"].asDouble() == 3.5 && w["mask"].asString() == "hard" &&
				  w["fft_size"].asInt() == 512 && w["time_span"].asInt() == 3 && w["freq_span"].asInt() == 0,
			  "every key written");
		c.deserialize(w);
		CHECK(all(c), "round trip");
		a.deserialize(Json::Value());
		CHECK(a.harmonic_db == 0 && a.percussive_db == -120 && a.mask == Audio_separation::Mask::Soft && a.time_span == 8 && a.serialize().isNull(),
			  "absent keys are their defaults again");
	}
	{
		Audio_separation a;
		a.deserialize(with("fft_size", 2048));
		a.deserialize(with("time_span", 8));
		a.deserialize(with("mask", "soft"));
		a.deserialize(with("percussive_db", -120.0));
		CHECK(a.serialize().isNull(), "the defaults, spelled out, are not written back");
		a.deserialize(with("freq_span", 4));
		CHECK(a.serialize().size() == 1 && a.serialize()["freq_span"].asInt() == 4, "only non-defaults written");
	}
	for (const char* key : real_keys)
	{
		CHECK(rejects_keeping(with(key, -120.5), key) && rejects_keeping(with(key, 12.5), key), key << ": values outside the range rejected");
		CHECK(rejects_keeping(with(key, "loud"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_separation a;
		a.deserialize(with(key, -120.0));
		CHECK((key == std::string("harmonic_db") ? a.harmonic_db : a.percussive_db) == -120, key << ": the lower limit itself is accepted");
		a.deserialize(with(key, 12.0));
		CHECK(a.serialize()[key].asDouble() == 12, key << ": the upper limit itself is accepted");
	}
	for (const char* key : int_keys)
	{
		CHECK(rejects_keeping(with(key, -1), key) && rejects_keeping(with(key, NAE_HPSS_MAX_SPAN + 1), key) && rejects_keeping(with(key, 1.5), key) &&
				  rejects_keeping(with(key, 1e12), key),
			  key << ": values outside the range, a fraction and a number beyond int rejected");
		CHECK(rejects_keeping(with(key, "wide"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_separation a;
		a.deserialize(with(key, 0));
		CHECK(a.serialize()[key].asInt() == 0, key << ": 0 is accepted");
		a.deserialize(with(key, NAE_HPSS_MAX_SPAN));
		CHECK(a.serialize().isNull(), key << ": the upper limit itself is accepted, and is the default");
	}
	CHECK(rejects_keeping(with("mask", "medium"), "mask") && rejects_keeping(with("mask", 1), "mask") && rejects_keeping(with("mask", true), "mask"),
		  "mask: an unknown name, a number and a bool rejected");
	for (const int n : {512, 1024, 4096})
	{
		Audio_separation a;
		a.deserialize(with("fft_size", n));
		CHECK(a.fft_size == n && a.serialize()["fft_size"].asInt() == n, "fft_size " << n << " accepted");
	}
	CHECK(rejects_keeping(with("fft_size", 256), "fft_size") && rejects_keeping(with("fft_size", 8192), "fft_size") &&
			  rejects_keeping(with("fft_size", 1000), "fft_size") && rejects_keeping(with("fft_size", 1024.5), "fft_size") &&
			  rejects_keeping(with("fft_size", "2048"), "fft_size") && rejects_keeping(with("fft_size", true), "fft_size"),
		  "fft_size: other sizes, a fraction, a string and a bool rejected");
	{
		// the headless draw_content keeps what the widgets would
		Audio_separation a;
		a.harmonic_db = 60;
		a.percussive_db = -200;
		a.time_span = 12;
		a.freq_span = -3;
		a.fft_size = 1000;
		CHECK(a.draw_content(false) == false && a.harmonic_db == 12 && a.percussive_db == -120 && a.time_span == 8 && a.freq_span == 0 && a.fft_size == 2048,
			  "draw_content: values in range");
	}
}

// the thirteen existing calls keep their counts; the fourteenth adds audio_separation
static void test_registry()
{
	const auto& map = infra::Processor::processor_map;
	for (const Registration& r : registrations)
	{
		r.call();
		CHECK(map.size() == r.count, "behind the call that adds " << (*r.adds ? r.adds : "the reference's list") << ": " << map.size() << " entries, not " << r.count);
	}
	infra::register_multiband_processors();
	print_registry();
	CHECK(map.size() == 19 && map.count("audio_multiband") == 1 && map.count("audio_separation") == 0, "no audio_separation before its call: " << map.size() << " entries");
	infra::register_separation_processors();
	print_registry();
	CHECK(map.size() == 20 && map.count("audio_separation") == 1, "audio_separation behind its call: " << map.size() << " entries");
	check_generated("audio_separation");
}

// a two-tone chord under a click every 3000 samples, the right channel quieter, on a little noise
static std::vector<float> signal(size_t frames)
{
	std::vector<float> x = uniform_noise(frames * 2);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < 2; c++)
		{
			const double tone = 0.25 * std::sin(0.0576 * (double)n) + 0.25 * std::sin(0.0864 * (double)n + 1.0);
			const double click = n % 3000 == 1500 ? 0.9 : 0.0;
			x[n * 2 + c] = (float)(((double)x[n * 2 + c] * 0.001 + tone + click) * (c ? 0.5 : 1.0));
		}
	return x;
}

static void graph_case(const Json::Value& json, double harmonic_db, double percussive_db, int n_fft, int tn, int fn, int hard, const char* what, bool removes_clicks)
{
	const int S = 30000, frame_size = 1152;
	const std::vector<float> x = signal(S);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_separation>(x, json, frame_size, sink, &error);
	CHECK(ok, "source -> audio_separation -> sink runs: " << error);
	if (!ok) return;
	nae_hpss_params params;
	CHECK(nae_hpss_design(harmonic_db, percussive_db, n_fft, tn, fn, hard, &params) == 0, "design");
	const std::vector<float> y = block_call(x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) {
		int rc = nae_hpss_block_f32(ctx, &params, sx, S, 2, 1, sy);
		if (rc == 0) rc = nae_sync(ctx);
		return rc;
	});
	if (y.empty()) return;
	if (removes_clicks)
	{
		// at the clicks' own samples what stands above the chord is 0.9 in the input
		double in_e = 0, out_e = 0;
		for (size_t n = 1500; n < (size_t)S; n += 3000)
		{
			const double tone = 0.25 * std::sin(0.0576 * (double)n) + 0.25 * std::sin(0.0864 * (double)n + 1.0);
			in_e += ((double)x[n * 2] - tone) * ((double)x[n * 2] - tone);
			out_e += ((double)y[n * 2] - tone) * ((double)y[n * 2] - tone);
		}
		CHECK(out_e < 0.1 * in_e, "the defaults take the clicks down by more than 10 dB at their own samples: " << out_e / in_e);
	}
	check_frames(*sink, y, S, frame_size, what);
}

static void test_gpu()
{
	graph_case(Json::Value(), 0, -120, 2048, 8, 8, 0, "the defaults: the block call's samples", true);
	Json::Value v;
	v["harmonic_db"] = -120.0;
	v["percussive_db"] = 3.0;
	v["mask"] = "hard";
	v["fft_size"] = 512;
	v["time_span"] = 3;
	v["freq_span"] = 5;
	graph_case(v, -120, 3, 512, 3, 5, 1, "the percussive part, hard mask, 512: the block call's samples", false);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "HPSS", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}});
}
