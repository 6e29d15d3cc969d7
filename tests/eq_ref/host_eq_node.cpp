// host_eq_node.cpp — the host mirror's equalizer node (tests/test_eq_cpu.py and tests/test_gpu_eq.py build it through tests/node_harness.py).
// `json`: no GPU — every key of audio_eq round-trips, the defaults are not written back, wrong values are rejected with their key, and the
// JSON arrays of json_mini.hpp behave as JsonCpp's.  `registry`: no GPU — the processor map after the three existing registration calls and
// after register_equalizer_processors().  `gpu`: a source -> audio_eq -> sink graph delivers the frames it received, with their sizes and pts,
// and the samples of nae_eq_block_f32 with the designed coefficients, bit for bit.  `wire`: an empty "bands" delivers the input's bits.
// `wire_s16`: no kernel runs — without bands a packed S16 stream arrives as it was sent, format, sizes, pts and words.
// `nyquist`: a band at or above half the sample rate fails the run on the first frame.
#include "../node_harness.hpp"
#include "processor/audio-eq.hpp"
#include "nae_dsp_spec.h"

using Kind = Audio_eq::Kind;
using Band = Audio_eq::Band;

static const char* kinds[] = {"peak", "lowshelf", "highshelf", "lowpass", "highpass", "notch"};

static Json::Value one_band(const Json::Value& band)
{
	Json::Value v, list(Json::arrayValue);
	list.append(band);
	v["bands"] = list;
	return v;
}

// a rejected value leaves the node as it was
static bool rejects_keeping(const Json::Value& v, const std::string& field)
{
	Audio_eq node;
	Json::Value b;
	b["freq"] = 440;
	node.deserialize(one_band(b));
	return rejects(node, v, field) && node.bands.size() == 1 && node.bands[0].freq == 440;
}

static void test_json_arrays()
{
	Json::Value a(Json::arrayValue), n, o;
	CHECK(a.isArray() && a.size() == 0 && !a.isNull(), "an empty array is an array of size 0, not null");
	CHECK(!n.isArray() && n.isNull() && n.size() == 0, "a null value is no array");
	a.append(Json::Value(3));
	a.append(Json::Value("x"));
	const Json::Value& ca = a;
	CHECK(a.size() == 2 && a[0].asInt() == 3 && a[1].asString() == "x" && ca[2].isNull() && a.size() == 2, "append, operator[](int), size()");
	o["k"] = 1;
	o["l"] = 2;
	CHECK(!o.isArray() && o.size() == 2, "an object's size() stays its member count");
	n.append(Json::Value(1.5));
	CHECK(n.isArray() && n.size() == 1 && n[0].asDouble() == 1.5, "append turns a null value into an array");
	o["list"] = a;
	const Json::Value& c = o;
	CHECK(c["list"].isArray() && c["list"].size() == 2 && c["list"][1].asString() == "x", "an array as a member, read through const");
}

static void test_json()
{
	test_json_arrays();
	Audio_eq node;
	CHECK(node.bands.empty() && node.serialize().isNull(), "defaults: no bands, nothing written");
	node.deserialize(Json::Value());
	CHECK(node.bands.empty() && node.serialize().isNull(), "a project without the key is a wire");
	{
		Json::Value v;
		v["bands"] = Json::Value(Json::arrayValue);
		node.deserialize(v);
		CHECK(node.bands.empty() && node.serialize().isNull(), "an empty bands is a wire, and is not written back");
	}
	for (int k = 0; k < 6; k++)
	{
		Json::Value b;
		b["kind"] = kinds[k];
		b["freq"] = 250.5;
		b["gain_db"] = -7.25;
		b["q"] = 3;
		Audio_eq a, c;
		a.deserialize(one_band(b));
		CHECK(a.bands.size() == 1 && (int)a.bands[0].kind == k && a.bands[0].freq == 250.5 && a.bands[0].gain_db == -7.25 && a.bands[0].q == 3, "read " << kinds[k]);
		const Json::Value w = a.serialize();
		CHECK(w["bands"].isArray() && w["bands"].size() == 1, "one band written");
		const Json::Value& wb = w["bands"][0];
		CHECK(wb.isMember("kind") == (k != 0) && wb["freq"].asDouble() == 250.5 && wb["gain_db"].asDouble() == -7.25 && wb["q"].asDouble() == 3, "written " << kinds[k]);
		c.deserialize(w);
		CHECK(c.bands.size() == 1 && c.bands[0].kind == a.bands[0].kind && c.bands[0].freq == 250.5 && c.bands[0].gain_db == -7.25 && c.bands[0].q == 3, "round trip");
	}
	{
		// a band of defaults is written as an empty object and read back as one band; 16 bands keep their order
		Json::Value v, list(Json::arrayValue);
		for (int i = 0; i < 16; i++)
		{
			Json::Value b;
			if (i) b["freq"] = 100.0 * i;
			list.append(b);
		}
		v["bands"] = list;
		Audio_eq a, c;
		a.deserialize(v);
		CHECK(a.bands.size() == 16 && a.bands[0].kind == Kind::Peak && a.bands[0].freq == 1000 && a.bands[0].gain_db == 0 && a.bands[0].q == 0.707, "defaults peak / 1000 / 0 / 0.707");
		const Json::Value w = a.serialize();
		CHECK(w["bands"].size() == 16 && w["bands"][0].isNull() && w["bands"][0].size() == 0, "defaults are not written back");
		CHECK(!w["bands"][5].isMember("kind") && !w["bands"][5].isMember("q") && !w["bands"][5].isMember("gain_db") && w["bands"][5]["freq"].asDouble() == 500, "only non-defaults written");
		c.deserialize(w);
		bool same = c.bands.size() == 16;
		for (int i = 0; same && i < 16; i++) same = c.bands[i].freq == a.bands[i].freq;
		CHECK(same, "16 bands round-trip in order");
		list.append(Json::Value());
		v["bands"] = list;
		CHECK(rejects_keeping(v, "bands"), "17 bands rejected");
	}
	{
		Json::Value s, n, o, e(Json::arrayValue), l(Json::arrayValue);
		s["bands"] = "many";
		n["bands"] = 3;
		o["bands"]["freq"] = 100;     // an object where the array belongs
		e.append(Json::Value(5));     // an entry that is no object
		l.append(Json::Value(Json::arrayValue));
		Json::Value ve, vl;
		ve["bands"] = e;
		vl["bands"] = l;
		CHECK(rejects_keeping(s, "bands") && rejects_keeping(n, "bands") && rejects_keeping(o, "bands") && rejects_keeping(ve, "bands") && rejects_keeping(vl, "bands"),
			  "bands: a string, a number, an object, a number entry and an array entry rejected");
	}
	{
		Json::Value a, b;
		a["kind"] = 1;
		b["kind"] = "bandpass";
		CHECK(rejects_keeping(one_band(a), "kind") && rejects_keeping(one_band(b), "kind"), "kind: a number and an unknown name rejected");
	}
	for (double f : {0.0, -20.0})
	{
		Json::Value b;
		b["freq"] = f;
		CHECK(rejects_keeping(one_band(b), "freq"), "freq " << f << " rejected");
	}
	for (double g : {24.5, -24.5, 1e9})
	{
		Json::Value b;
		b["gain_db"] = g;
		CHECK(rejects_keeping(one_band(b), "gain_db"), "gain_db " << g << " rejected");
	}
	for (double q : {0.0, 0.05, 40.5, -1.0})
	{
		Json::Value b;
		b["q"] = q;
		CHECK(rejects_keeping(one_band(b), "q"), "q " << q << " rejected");
	}
	for (const char* key : {"freq", "gain_db", "q"})
	{
		Json::Value b;
		b[key] = "loud";
		CHECK(rejects_keeping(one_band(b), key), key << ": a string rejected");
	}
	{
		Json::Value lo, hi;
		lo["gain_db"] = -24;
		lo["q"] = 0.1;
		hi["gain_db"] = 24;
		hi["q"] = 40;
		Audio_eq a;
		a.deserialize(one_band(lo));
		a.deserialize(one_band(hi));
		CHECK(a.bands.size() == 1 && a.bands[0].gain_db == 24 && a.bands[0].q == 40, "the limits themselves are accepted");
	}
	{
		// the headless draw_content keeps what the widgets would
		Audio_eq a;
		a.bands.resize(20);
		a.bands[0].gain_db = 30;
		a.bands[1].q = 100;
		CHECK(a.draw_content(false) == false && a.bands.size() == 16 && a.bands[0].gain_db == 24 && a.bands[1].q == 40, "draw_content: 16 bands, values in range");
	}
}

static void test_registry() { check_registry("audio_eq"); }

struct Band_spec { const char* kind; double freq, gain_db, q; };
static const Band_spec graph_bands[] = {{"highpass", 40, 0, 0.7071}, {"peak", 1000, 6, 1}, {"lowshelf", 150, -4, 0.707}, {"notch", 50, 0, 30}, {"highshelf", 9000, 3, 0.9}};

static Json::Value graph_json()
{
	Json::Value v, list(Json::arrayValue);
	for (const auto& s : graph_bands)
	{
		Json::Value b;
		b["kind"] = s.kind;
		b["freq"] = s.freq;
		b["gain_db"] = s.gain_db;
		b["q"] = s.q;
		list.append(b);
	}
	v["bands"] = list;
	return v;
}

static void test_gpu()
{
	const int S = 20000, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_eq>(x, graph_json(), frame_size, sink, &error);
	CHECK(ok, "source -> audio_eq -> sink runs: " << error);
	if (!ok) return;
	// the block call on the same samples with the designed coefficients
	constexpr int n_bands = sizeof(graph_bands) / sizeof(graph_bands[0]);
	double coef[n_bands * 5];
	for (int i = 0; i < n_bands; i++)
	{
		int k = 0;
		while (std::string(kinds[k]) != graph_bands[i].kind) k++;
		CHECK(nae_eq_design(k, 48000, graph_bands[i].freq, graph_bands[i].gain_db, graph_bands[i].q, coef + 5 * i) == 0, "design");
	}
	const std::vector<float> y = block_call(x, S, [&](nae_ctx* ctx, const nae_sig* sx, const nae_sig* sy) { return nae_eq_block_f32(ctx, coef, n_bands, sx, S, 2, 1, sy); });
	if (y.empty()) return;
	check_frames(*sink, y, S, frame_size, "the block call's samples with the designed coefficients");
}

static void test_wire()
{
	const int S = 5000, frame_size = 1152;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	for (int empty = 0; empty < 2; empty++)
	{
		Json::Value v;
		if (empty) v["bands"] = Json::Value(Json::arrayValue);
		std::shared_ptr<Sink> sink;
		std::string error;
		const bool ok = run_graph<Audio_eq>(x, v, frame_size, sink, &error);
		CHECK(ok, "the wire runs: " << error);
		if (ok) check_frames(*sink, x, S, frame_size, empty ? "empty bands: the input's bits" : "absent bands: the input's bits");
	}
}

// the wire converts nothing: 2500 samples of packed S16 in frames of 1000 arrive as 1000 / 1000 / 500 of S16, pts and words unchanged
static void test_wire_s16()
{
	const int S = 2500, frame_size = 1000;
	const std::vector<float> x = uniform_noise((size_t)S * 2);
	const std::vector<int16_t> sent = quantise_s16(x.data(), x.size());
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_eq>(x, Json::Value(), frame_size, sink, &error, 48000, AV_SAMPLE_FMT_S16);
	CHECK(ok, "the wire runs: " << error);
	if (!ok) return;
	CHECK(sink->frames.size() == 3, "as many frames as the source sent: " << sink->frames.size());
	const int sizes[] = {1000, 1000, 500};
	size_t pos = 0;
	for (size_t f = 0; f < sink->frames.size() && f < 3; f++)
	{
		const Frame_data* d = sink->frames[f]->data();
		const int64_t want_pts = (int64_t)((0.5 + double(f * frame_size) / 48000) * 1000000);   // the source's own formula
		const bool shape_ok = d->format == AV_SAMPLE_FMT_S16 && d->nb_samples == sizes[f] && d->ch_layout.nb_channels == 2 && d->sample_rate == 48000 &&
							  d->pts == want_pts && d->time_base.num == 1 && d->time_base.den == 1000000;
		CHECK(shape_ok, "frame " << f << ": S16, " << sizes[f] << " samples, the source's pts and time base");
		if (!shape_ok) return;
		CHECK(std::memcmp(d->data[0], sent.data() + pos * 2, (size_t)sizes[f] * 2 * sizeof(int16_t)) == 0, "frame " << f << ": the words the source sent");
		pos += sizes[f];
	}
}

static void test_nyquist()
{
	const std::vector<float> x = uniform_noise(4000);
	Json::Value b;
	b["freq"] = 24000;    // Nyquist at the source's 48 kHz
	std::shared_ptr<Sink> sink;
	std::string error;
	const bool ok = run_graph<Audio_eq>(x, one_band(b), 1152, sink, &error);
	CHECK(!ok && error.find("band 0") != std::string::npos, "a band at Nyquist fails the run on the first frame: " << error);
}

int main(int argc, char** argv)
{
	return harness_main(argc, argv, "EQ", {{"json", test_json}, {"registry", test_registry}, {"gpu", test_gpu}, {"wire", test_wire}, {"wire_s16", test_wire_s16}, {"nyquist", test_nyquist}});
}
