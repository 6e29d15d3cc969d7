// host_denoise_node.cpp — the host mirror's noise reduction node (tests/test_denoise_cpu.py and tests/test_gpu_denoise.py build it through
// tests/node_harness.py).  `json`: no GPU — every key of audio_denoise round-trips, the defaults are not written back, wrong values are rejected
// with their key.  `registry`: no GPU — the processor map after the five existing registration calls and after
// register_restoration_processors().  `gpu`: a source -> audio_denoise -> sink graph delivers the frames it received, with their sizes and pts,
// and the samples of nae_denoise_block_f32 with the profile nae_denoise_profile_f32 learns from the stretch, bit for bit.  `short`: a stream
// that ends with fewer than fft_size samples in the stretch fails the run.
#include "../node_harness.hpp"
#include "processor/audio-denoise.hpp"
#include "nae_dsp_spec.h"

static const char* real_keys[] = {"reduction_db", "sensitivity_db", "profile_start_ms", "profile_ms"};
static const char* int_keys[] = {"time_smooth", "freq_smooth"};

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_denoise node;
	Json::Value b;
	b["reduction_db"] = 7;
	node.deserialize(b);
	return rejects(node, v, field) && node.reduction_db == 7 && node.fft_size == 2048 && node.time_smooth == 2;
}

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

static void test_json()
{
	Audio_denoise node;
	CHECK(node.reduction_db == 12 && node.sensitivity_db == 6 && node.fft_size == 2048 && node.time_smooth == 2 && node.freq_smooth == 2 &&
			  node.profile_start_ms == 0 && node.profile_ms == 500,
		  "defaults: 12 dB, 6 dB, 2048, 2 frames, 2 bins, the first 500 ms");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	node.deserialize(Json::Value());
	CHECK(node.serialize().isNull() && node.fft_size == 2048, "a project without the keys keeps the defaults");
	{
		Json::Value v;
		v["reduction_db"] = 24.5;
		v["sensitivity_db"] = -2.25;
		v["fft_size"] = 512;
		v["time_smooth"] = 8;
		v["freq_smooth"] = 0;
		v["profile_start_ms"] = 1250.5;
		v["profile_ms"] = 20;
		Audio_denoise a, c;
		a.deserialize(v);
		CHECK(a.reduction_db == 24.5 && a.sensitivity_db == -2.25 && a.fft_size == 512 && a.time_smooth == 8 && a.freq_smooth == 0 &&
				  a.profile_start_ms == 1250.5 && a.profile_ms == 20,
			  "every key read");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 7 && w["reduction_db"].asDouble() == 24.5 && w["sensitivity_db"].asDouble() == -2.25 && w["fft_size"].asInt() == 512 &&
				  w["time_smooth"].asInt() == 8 && w["freq_smooth"].asInt() == 0 && w["profile_start_ms"].asDouble() == 1250.5 && w["profile_ms"].asDouble() == 20,
			  "every key written");
		c.deserialize(w);
		CHECK(c.reduction_db == a.reduction_db && c.sensitivity_db == a.sensitivity_db && c.fft_size == a.fft_size && c.time_smooth == a.time_smooth &&
				  c.freq_smooth == a.freq_smooth && c.profile_start_ms == a.profile_start_ms && c.profile_ms == a.profile_ms,
			  "round trip");
		a.deserialize(Json::Value());
		CHECK(a.reduction_db == 12 && a.fft_size == 2048 && a.freq_smooth == 2 && a.serialize().isNull(), "absent keys are their defaults again");
	}
	{
		Audio_denoise a;
		a.deserialize(with("fft_size", 2048));
		a.deserialize(with("time_smooth", 2));
		CHECK(a.serialize().isNull(), "the defaults, spelled out, are not written back");
		a.deserialize(with("freq_smooth", 4));
		CHECK(a.serialize().size() == 1 && a.serialize()["freq_smooth"].asInt() == 4, "only non-defaults written");
	}
	const double below[] = {-0.5, -6.5, -0.5, 19.5}, above[] = {48.5, 24.5, 60000.5, 10000.5};
	const double lo[] = {0, -6, 0, 20}, hi[] = {48, 24, 60000, 10000};
	for (int i = 0; i < 4; i++)
	{
		const char* key = real_keys[i];
		CHECK(rejects_keeping(with(key, below[i]), key) && rejects_keeping(with(key, above[i]), key), key << ": values outside the range rejected");
		CHECK(rejects_keeping(with(key, "loud"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_denoise a;
		a.deserialize(with(key, lo[i]));
		CHECK(a.serialize()[key].asDouble() == lo[i] || lo[i] == 0, key << ": the lower limit itself is accepted");
		a.deserialize(with(key, hi[i]));
		CHECK(a.serialize()[key].asDouble() == hi[i], key << ": the upper limit itself is accepted");
	}
	const int int_hi[] = {NAE_DENOISE_MAX_TIME, NAE_DENOISE_MAX_FREQ};
	for (int i = 0; i < 2; i++)
	{
		const char* key = int_keys[i];
		CHECK(rejects_keeping(with(key, -1), key) && rejects_keeping(with(key, int_hi[i] + 1), key) && rejects_keeping(with(key, 1.5), key) &&
				  rejects_keeping(with(key, 1e12), key),
			  key << ": values outside the range, a fraction and a number beyond int rejected");
		CHECK(rejects_keeping(with(key, "wide"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_denoise a;
		a.deserialize(with(key, 0));
		CHECK(a.serialize()[key].asInt() == 0, key << ": 0 is accepted");
		a.deserialize(with(key, int_hi[i]));
		CHECK(a.serialize()[key].asInt() == int_hi[i], key << ": the upper limit itself is accepted");
	}
	for (const int n : {512, 1024, 4096})
	{
		Audio_denoise a;
		a.deserialize(with("fft_size", n));
		CHECK(a.fft_size == n && a.serialize()["fft_size"].asInt() == n, "fft_size " << n << " accepted");
	}
	CHECK(rejects_keeping(with("fft_size", 256), "fft_size") && rejects_keeping(with("fft_size", 8192), "fft_size") &&
			  rejects_keeping(with("fft_size", 1000), "fft_size") && rejects_keeping(with("fft_size", 1024.5), "fft_size") &&
			  rejects_keeping(with("fft_size", "2048"), "fft_size") && rejects_keeping(with("fft_size", true), "fft_size"),
		  "fft_size: other sizes, a fraction, a string and a bool rejected");
	{
		// the headless draw_content keeps what the widgets would
		Audio_denoise a;
		a.reduction_db = 60;
		a.time_smooth = 12;
		a.fft_size = 1000;
		a.profile_ms = 1;
		CHECK(a.draw_content(false) == false && a.reduction_db == 48 && a.time_smooth == 8 && a.fft_size == 2048 && a.profile_ms == 20, "draw_content: values in range");
	}
}

static void test_registry() { check_registry("audio_denoise"); }

// a lead-in of quiet noise, then the same noise under a two-tone, the right channel quieter
static std::vector<float> signal(size_t frames, size_t lead)
{
	std::vector<float> x = uniform_noise(frames * 2);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < 2; c++)
		{
			const double tone = n < lead ? 0.0 : 0.4 * std::sin(0.13 * (double)n) + 0.2 * std::sin(0.71 * (double)n + 1.0);
			x[n * 2 + c] = (float)(((double)x[n * 2 + c] * 0.01 + tone) * (c ? 0.5 : 1.0));
		}
	return x;
}

static Json::Value graph_json(int fft_size, double start_ms, double len_ms)
{
	Json::Value v;
	v["reduction_db"] = 18;
	v["sensitivity_db"] = 9;
	v["fft_size"] = fft_size;
	v["time_smooth"] = 3;
	v["freq_smooth"] = 1;
	v["profile_start_ms"] = start_ms;
	v["profile_ms"] = len_ms;
	return v;
}

static void test_gpu()
{
	const int S = 30000, frame_size = 1152;
	const std::vector<float> x = signal(S, 9000);
	// the stretch 25 ms ... 175 ms is 1200 ... 8400 at 48 kHz; a stretch that reaches past the end of the stream is cut there
	const struct { int n_fft; double start_ms, len_ms; size_t start, len; } cases[] = {{1024, 25, 150, 1200, 7200}, {512, 600, 1000, 28800, 1200}};
	for (const auto& k : cases)
	{
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph<Audio_denoise>(x, graph_json(k.n_fft, k.start_ms, k.len_ms), frame_size, sink, &error);
		CHECK(ok, "source -> audio_denoise -> sink runs: " << error);
		if (!ok) return;
		nae_denoise_params params;
		CHECK(nae_denoise_design(18, 9, k.n_fft, 3, 1, &params) == 0, "design");
		const std::vector<float> y = block_call(x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) {
			void* d_profile = nullptr;
			if (nae_malloc(ctx, 2 * (size_t)(k.n_fft / 2 + 1) * sizeof(float), &d_profile) != 0) return -100;
			const nae_sig excerpt{static_cast<float*>(sx->base) + k.start * 2, 0, 1, 2};
			int rc = nae_denoise_profile_f32(ctx, k.n_fft, &excerpt, k.len, 2, static_cast<float*>(d_profile));
			if (rc == 0) rc = nae_denoise_block_f32(ctx, &params, static_cast<float*>(d_profile), 2, sx, S, 2, 1, sy);
			if (rc == 0) rc = nae_sync(ctx);
			nae_free(ctx, d_profile);
			return rc;
		});
		if (y.empty()) return;
		double in_e = 0, out_e = 0;
		for (size_t i = 0; i < 2 * 8000; i++) { in_e += (double)x[i] * x[i]; out_e += (double)y[i] * y[i]; }
		CHECK(out_e < 0.1 * in_e, "the graph's parameters turn the lead-in down: " << out_e / in_e);
		check_frames(*sink, y, S, frame_size, "the block call's samples with the learned profile");
	}
}

static void test_short()
{
	const std::vector<float> x = signal(3000, 3000);
	// 2048-sample frames, and the stream ends 1800 samples into the stretch
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_denoise>(x, graph_json(2048, 25, 500), 1152, sink, &error);
	CHECK(!ok && error.find("1800 samples of the stretch") != std::string::npos, "a stretch shorter than one frame fails the run: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "DENOISE", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"short", test_short}});
}
