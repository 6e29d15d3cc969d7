// host_dynkey_node.cpp — the host mirror's side-chain node (tests/test_dynkey_cpu.py and tests/test_gpu_dynkey.py build it through
// tests/node_harness.py).  `json`: no GPU — audio_dynamics' nine keys and "key_filter" round-trip, the defaults are not written back, wrong
// values are rejected with their key.  `registry`: no GPU — the processor map after the seven existing registration calls and after
// register_sidechain_processors(); the node has three pins, two of them audio inputs.  `gpu`: two sources -> audio_sidechain -> sink with the
// key 100 samples late, 37 samples early, ending before the input, and not linked at all: the input's frames, sizes and pts, and the samples
// of nae_dynkey_block_f32 on the arrays lined up by the pts rule, bit for bit.  `errors`: a key of another sample rate, a key with more
// channels than the input, a look-ahead of more than 1024 samples and a filter band above Nyquist fail the run on the first frames.
#include "../node_harness.hpp"
#include "processor/audio-sidechain.hpp"
#include "nae_dsp_spec.h"

using Mode = Dynamics_settings::Mode;

static Json::Value with(const char* key, const Json::Value& v)
{
	Json::Value o;
	o[key] = v;
	return o;
}

static Json::Value band(const char* kind, double freq, double q)
{
	Json::Value b;
	b["kind"] = kind;
	b["freq"] = freq;
	b["q"] = q;
	return b;
}

static Json::Value filter_of(int n)
{
	Json::Value list(Json::arrayValue);
	for (int i = 0; i < n; i++) list.append(band(i & 1 ? "peak" : "highpass", 200.0 * (i + 1), 0.9));
	return list;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_sidechain node;
	Json::Value b;
	b["ratio"] = 7;
	b["key_filter"] = filter_of(2);
	node.deserialize(b);
	return rejects(node, v, field) && node.dynamics.ratio == 7 && node.dynamics.mode == Mode::Compressor && node.key_filter.size() == 2;
}

static void test_json()
{
	Audio_sidechain node;
	CHECK(node.dynamics.mode == Mode::Compressor && node.dynamics.threshold_db == -18 && node.dynamics.ratio == 4 && node.dynamics.knee_db == 6 &&
			  node.dynamics.attack_ms == 5 && node.dynamics.release_ms == 100 && node.dynamics.lookahead_ms == 0 && node.dynamics.makeup_db == 0 &&
			  node.dynamics.link_channels && node.key_filter.empty(),
		  "defaults: audio_dynamics', and no key filter");
	CHECK(node.serialize().isNull(), "defaults are not written back");
	{
		Json::Value v;
		v["mode"] = "limiter";
		v["threshold_db"] = -3.5;
		v["ratio"] = 20;
		v["knee_db"] = 0;
		v["attack_ms"] = 0.25;
		v["release_ms"] = 250;
		v["lookahead_ms"] = 1.5;
		v["makeup_db"] = 2.25;
		v["link_channels"] = false;
		v["key_filter"] = filter_of(4);
		Audio_sidechain a, c;
		a.deserialize(v);
		CHECK(a.dynamics.mode == Mode::Limiter && a.dynamics.threshold_db == -3.5 && a.dynamics.ratio == 20 && a.dynamics.knee_db == 0 &&
				  a.dynamics.attack_ms == 0.25 && a.dynamics.release_ms == 250 && a.dynamics.lookahead_ms == 1.5 && a.dynamics.makeup_db == 2.25 &&
				  !a.dynamics.link_channels,
			  "the nine keys read");
		CHECK(a.key_filter.size() == 4 && a.key_filter[0].kind == Audio_eq::Kind::Highpass && a.key_filter[1].kind == Audio_eq::Kind::Peak &&
				  a.key_filter[3].freq == 800 && a.key_filter[2].q == 0.9 && a.key_filter[0].gain_db == 0,
			  "key_filter read in audio_eq's format");
		const Json::Value w = a.serialize();
		CHECK(w.size() == 10 && w["mode"].asString() == "limiter" && w["ratio"].asDouble() == 20 && w["lookahead_ms"].asDouble() == 1.5 &&
				  !w["link_channels"].asBool() && w["key_filter"].size() == 4 && w["key_filter"][0]["kind"].asString() == "highpass" &&
				  !w["key_filter"][1].isMember("kind") && w["key_filter"][1]["freq"].asDouble() == 400,
			  "every key written, a band's defaults left out");
		c.deserialize(w);
		CHECK(c.dynamics.mode == a.dynamics.mode && c.dynamics.threshold_db == a.dynamics.threshold_db && c.dynamics.release_ms == a.dynamics.release_ms &&
				  c.key_filter.size() == 4 && c.key_filter[3].freq == 800 && c.key_filter[0].kind == Audio_eq::Kind::Highpass,
			  "round trip");
		a.deserialize(Json::Value());
		CHECK(a.dynamics.mode == Mode::Compressor && a.dynamics.ratio == 4 && a.key_filter.empty() && a.serialize().isNull(), "absent keys are their defaults again");
	}
	{
		Audio_sidechain a;
		a.deserialize(with("key_filter", filter_of(0)));
		CHECK(a.key_filter.empty() && a.serialize().isNull(), "an empty key_filter is none, and is not written back");
		a.deserialize(with("key_filter", filter_of(1)));
		CHECK(a.serialize().size() == 1 && a.serialize()["key_filter"].size() == 1, "only non-defaults written");
	}
	CHECK(rejects_keeping(with("key_filter", filter_of(5)), "key_filter"), "five bands rejected");
	CHECK(rejects_keeping(with("key_filter", 3), "key_filter") && rejects_keeping(with("key_filter", "highpass"), "key_filter") &&
			  rejects_keeping(with("key_filter", band("peak", 100, 1)), "key_filter"),
		  "key_filter: a number, a string and a lone band rejected");
	{
		Json::Value list(Json::arrayValue);
		list.append(7);
		CHECK(rejects_keeping(with("key_filter", list), "key_filter"), "an entry that is no object rejected");
		Json::Value bad(Json::arrayValue);
		bad.append(band("bell", 100, 1));
		CHECK(rejects_keeping(with("key_filter", bad), "kind"), "a band's unknown kind rejected with its key");
		Json::Value q(Json::arrayValue);
		q.append(band("peak", 100, 50));
		CHECK(rejects_keeping(with("key_filter", q), "q"), "a band's q outside its range rejected with its key");
		Json::Value fr(Json::arrayValue);
		fr.append(band("peak", 0, 1));
		CHECK(rejects_keeping(with("key_filter", fr), "freq"), "a band's frequency of 0 rejected with its key");
	}
	CHECK(rejects_keeping(with("mode", "expander"), "mode") && rejects_keeping(with("link_channels", 1), "link_channels"), "mode and link_channels as audio_dynamics'");
	const char* real_keys[] = {"threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "lookahead_ms", "makeup_db"};
	const double below[] = {-60.5, 0.5, -0.5, -0.5, 0.5, -0.5, -24.5}, above[] = {0.5, 100.5, 24.5, 500.5, 5000.5, 20.5, 24.5};
	const double lo[] = {-60, 1, 0, 0, 1, 0, -24}, hi[] = {0, 100, 24, 500, 5000, 20, 24};
	for (int i = 0; i < 7; i++)
	{
		const char* key = real_keys[i];
		CHECK(rejects_keeping(with(key, below[i]), key) && rejects_keeping(with(key, above[i]), key), key << ": values outside audio_dynamics' range rejected");
		CHECK(rejects_keeping(with(key, "loud"), key) && rejects_keeping(with(key, true), key), key << ": a string and a bool rejected");
		Audio_sidechain a;
		a.deserialize(with(key, lo[i]));
		a.deserialize(with(key, hi[i]));
		CHECK(a.serialize()[key].asDouble() == hi[i] || hi[i] == 0, key << ": the limits themselves are accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_sidechain a;
		a.dynamics.ratio = 500;
		a.key_filter.resize(6);
		a.key_filter[0].q = 100;
		CHECK(a.draw_content(false) == false && a.dynamics.ratio == 100 && a.key_filter.size() == 4 && a.key_filter[0].q == 40, "draw_content: values in range");
	}
}

// what the registry generates for the node: three pins
static void check_three_pins(const std::string& id)
{
	if (!infra::Processor::processor_map.count(id)) return;
	const auto node = infra::Processor::processor_map.at(id).generate();
	const auto pins = node->get_pin_attributes();
	int inputs = 0, outputs = 0;
	bool named = true;
	for (const auto& p : pins)
	{
		inputs += p.is_input && p.type.get() == typeid(Audio_stream);
		outputs += !p.is_input && p.type.get() == typeid(Audio_stream);
		named = named && (p.identifier == "input" || p.identifier == "key" || p.identifier == "output");
	}
	CHECK(node->get_processor_info_non_static().identifier == id && pins.size() == 3 && inputs == 2 && outputs == 1 && named,
		  "generate() gives the node: pins input, key and output, two of them audio inputs");
}

static void test_registry() { check_registry("audio_sidechain", check_three_pins); }

// the signal: plain noise at a steady level; the key: noise whose level swells from far under to over the threshold, the right channel quieter
static std::vector<float> key_noise(size_t frames, int ch)
{
	std::vector<float> x = uniform_noise(frames * ch, 99);
	for (size_t n = 0; n < frames; n++)
		for (int c = 0; c < ch; c++) x[n * ch + c] = (float)((double)x[n * ch + c] * (0.02 + 0.9 * (double)((n / 500) % 7) / 6.0) * (c ? 0.4 : 1.0));
	return x;
}

static Json::Value graph_json()
{
	Json::Value v;
	v["threshold_db"] = -20;
	v["ratio"] = 6;
	v["knee_db"] = 4;
	v["attack_ms"] = 1.5;
	v["release_ms"] = 60;
	v["lookahead_ms"] = 2.5;
	v["makeup_db"] = 3;
	Json::Value list(Json::arrayValue);
	list.append(band("highpass", 150, 0.7071));
	list.append(band("peak", 3000, 1.0));
	list[1]["gain_db"] = 6;
	v["key_filter"] = list;
	return v;
}

// input source (48 kHz stereo, pts from 0.5 s) and, with key_ch > 0, a key source -> audio_sidechain -> sink
static bool run_sidechain(const std::vector<float>& x, const std::vector<float>& key, int key_ch, double key_start, const Json::Value& json,
						  std::shared_ptr<Sink>& sink, std::string* error, int key_rate = 48000, int in_ch = 2, int key_frame = 1000, int in_rate = 48000)
{
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	src->frame_size = 1152;
	src->channels = in_ch;
	src->sample_rate = in_rate;
	auto node = std::make_shared<Audio_sidechain>();
	node->deserialize(json);
	sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(3, node); r.add_node(4, sink);
	r.add_link({1, "output", 3, "input"});
	r.add_link({3, "output", 4, "input"});
	if (key_ch)
	{
		auto ksrc = std::make_shared<Src>();
		ksrc->samples = key;
		ksrc->frame_size = key_frame;   // not the input's: the two pins' frames do not line up
		ksrc->channels = key_ch;
		ksrc->sample_rate = key_rate;
		ksrc->start_seconds = key_start;
		r.add_node(2, ksrc);
		r.add_link({2, "output", 3, "key"});
	}
	const bool ok = r.run();
	if (error) *error = r.get_processor_resources().at(3)->error_text;
	return ok;
}

static void test_gpu()
{
	const int S = 20000;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	struct Case { const char* what; int key_ch, key_len, offset; };
	// offset: the samples the key starts behind the input; a key that ends early is zero from there on
	const Case cases[] = {{"key 100 samples late", 2, S, 100}, {"key 37 samples early", 1, S, -37}, {"key ends before the input", 2, 9000, 0},
						  {"no key link", 0, 0, 0}};
	for (const Case& k : cases)
	{
		const std::vector<float> key = k.key_ch ? key_noise((size_t)k.key_len, k.key_ch) : std::vector<float>();
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_sidechain(x, key, k.key_ch, 0.5 + (double)k.offset / 48000.0, graph_json(), sink, &error);
		CHECK(ok, k.what << ": sources -> audio_sidechain -> sink runs: " << error);
		if (!ok) return;
		// the block call on the arrays lined up by the rule: the key sample for input sample n is key[n - o], zero outside the key
		nae_dynkey_params params{};
		CHECK(nae_dyn_design(48000, -20, 6, 4, 0.0015, 0.06, 0.0025, 3, 1, &params.dyn) == 0 && params.dyn.lookahead == 120, "design");
		params.key_ch = k.key_ch;
		params.n_sections = 2;
		CHECK(nae_eq_design(NAE_EQ_HIGHPASS, 48000, 150, 0, 0.7071, params.coef[0]) == 0 && nae_eq_design(NAE_EQ_PEAK, 48000, 3000, 6, 1.0, params.coef[1]) == 0, "sections");
		std::vector<float> both = x;   // the signal, and behind it the key as lined up
		both.resize((size_t)S * (2 + k.key_ch), 0.0f);
		for (int n = 0; n < S; n++)
		{
			const int j = n - k.offset;
			if (j >= 0 && j < k.key_len)
				for (int c = 0; c < k.key_ch; c++) both[(size_t)S * 2 + (size_t)n * k.key_ch + c] = key[(size_t)j * k.key_ch + c];
		}
		const std::vector<float> y = block_call(both, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) {
			const nae_sig skey{static_cast<float*>(sx->base) + (size_t)S * 2, 0, 1, (size_t)k.key_ch};
			return nae_dynkey_block_f32(ctx, &params, sx, k.key_ch ? &skey : nullptr, S, 2, 1, sy);
		});
		if (y.empty()) return;
		size_t changed = 0;
		for (size_t i = 0; i < y.size(); i++) changed += std::fabs(y[i]) < 0.8f * std::fabs(x[i]);
		CHECK(changed > y.size() / 10, k.what << ": the key compresses the signal: " << changed << " samples reduced");
		check_frames(*sink, y, S, 1152, k.what);
	}
}

static void test_errors()
{
	const std::vector<float> x = uniform_noise(4000 * 2), mono = uniform_noise(4000);
	const std::vector<float> key = key_noise(4000, 2);
	std::shared_ptr<Sink> sink;
	std::string error;
	bool ok = run_sidechain(x, key, 2, 0.5, graph_json(), sink, &error, 44100);
	CHECK(!ok && error.find("key 44100 Hz, input 48000 Hz") != std::string::npos, "a key of another sample rate fails the run: " << error);
	ok = run_sidechain(mono, key, 2, 0.5, graph_json(), sink, &error, 48000, 1);
	CHECK(!ok && error.find("key 2 channels, input 1") != std::string::npos, "a stereo key on a mono input fails the run: " << error);
	ok = run_sidechain(x, key, 2, 0.5, with("lookahead_ms", 20), sink, &error, 96000, 2, 1000, 96000);
	CHECK(!ok && error.find("lookahead 20 ms at 96000 Hz") != std::string::npos, "a look-ahead of 1920 samples fails the run: " << error);
	Json::Value list(Json::arrayValue);
	list.append(band("highpass", 30000, 0.7));
	ok = run_sidechain(x, key, 2, 0.5, with("key_filter", list), sink, &error);
	CHECK(!ok && error.find("band 0: 30000 Hz at 48000 Hz") != std::string::npos, "a key filter band above Nyquist fails the run: " << error);
	ok = run_sidechain(x, key, 1, 0.5, Json::Value(), sink, &error);
	CHECK(ok, "a mono key on a stereo input runs: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "DYNKEY", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"errors", test_errors}});
}
