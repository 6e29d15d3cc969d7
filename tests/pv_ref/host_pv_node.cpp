// host_pv_node.cpp — the host mirror's vocoder keys on Velocity_modifier and Pitch_modifier: "fft_size" (tests/test_pv_sizes_cpu.py,
// tests/test_gpu_pv_sizes.py), "phase_lock" (tests/test_pv_lock_cpu.py, tests/test_gpu_pv_lock.py), "transients"
// (tests/test_pv_transient_cpu.py, tests/test_gpu_pv_transient.py), "link_channels" (tests/test_pv_link_cpu.py, tests/test_gpu_pv_link.py) and,
// Pitch_modifier only, "formant" (tests/test_pv_formant_cpu.py, tests/test_gpu_pv_formant.py) and "formant_shift"
// (tests/test_pv_fshift_cpu.py, tests/test_gpu_pv_fshift.py).  Built by its tests with tests/node_harness.py.
//
// `json <key>`: no GPU.  The boolean keys (phase_lock, transients, link_channels, formant): absent means false and is not written; true
// round-trips; false is not written; a missing key resets; a value that is not a bool is "Wrong field: <key>"; with "algorithm": "soundtouch"
// the key is kept; then what each key combines with.  fft_size: a value that is not 512 / 1024 / 2048 / 4096, or a size other than 1024 with
// "phase_lock": true, is "Wrong field: fft_size".  formant_shift: a number of semitones round-trips (an integer too); 0 is not written; a value
// that is not a number is "Wrong field: formant_shift"; beyond +-24 it is a Runtime_error "Out of range: formant_shift"; Velocity_modifier
// ignores the key.
// `gpu <key> ...`: source -> Pitch_modifier -> sink through the fiber runner equals a block call on the same samples bit for bit, and differs
// from the block call without the key:
//   fft_size [out.f32]       {"pitch": 3, "fft_size": 4096} against nae_stretch_block_n_f32(4096)
//   phase_lock [out.f32]     {"pitch": 3, "phase_lock": true} against nae_stretch_block_ex_f32(NAE_STRETCH_PHASE_LOCK), not the unlocked call
//   formant [out.f32]        {"pitch": 4, "formant": true} against nae_stretch_block_formant_f32 with the node's lifter
//                            (these three write the input, then the graph's output, to out.f32 for the test's comparison with the CPU statement)
//   transients [lock]        {"pitch": 3, "fft_size": 2048, "transients": true} against nae_stretch_block_n_f32(2048, NAE_STRETCH_TRANSIENTS), not
//                            the unflagged call (clicks in both channels); lock: {"pitch": 3, "phase_lock": true, "transients": true} at 1024
//   link_channels [lock]     {"pitch": 3, "fft_size": 2048, "transients": true, "link_channels": true} against nae_stretch_block_n_f32(2048,
//                            NAE_STRETCH_TRANSIENTS | NAE_STRETCH_LINK_CHANNELS), not the call without the link (clicks in the left channel only);
//                            lock: {"pitch": 3, "phase_lock": true, "link_channels": true} at 1024
//   formant_shift <pitch> <shift> <in.f32> <out.f32>
//                            {"pitch": <pitch>, "formant_shift": <shift>} against nae_stretch_block_formant_shift_f32 (default lifter,
//                            formant_ratio 2^(shift / 12)), not the call without the shift; the input and the output are written for the caller
#include "../node_harness.hpp"
#include <cstdlib>
#include <functional>

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

// what every boolean key does on a node that has it
template <class Node>
static void json_bool_key(const char* name, const char* key)
{
	Node node;
	CHECK(!node.serialize().isMember(key), name << ": a default node writes no " << key);
	Json::Value on;
	on[key] = true;
	Node a;
	a.deserialize(on);
	const Json::Value w = a.serialize();
	CHECK(w.isMember(key) && w[key].isBool() && w[key].asBool(), name << ": true is written back");
	Node b;
	b.deserialize(w);
	CHECK(b.serialize()[key].isBool() && b.serialize()[key].asBool(), name << ": round trip");
	Json::Value off;
	off[key] = false;
	Node c;
	c.deserialize(off);
	CHECK(!c.serialize().isMember(key), name << ": false is not written");
	Node d;
	d.deserialize(on);
	d.deserialize(Json::Value());
	CHECK(!d.serialize().isMember(key), name << ": a missing key means false");
	for (const Json::Value& bad : {Json::Value(1), Json::Value(0), Json::Value(0.5), Json::Value(1.5), Json::Value("true")})
	{
		Json::Value v;
		v[key] = bad;
		CHECK(rejects<Node>(v, key), name << ": a " << key << " that is not a bool is rejected");
	}
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st[key] = true;
	Node e;
	e.deserialize(st);
	CHECK(e.serialize()[key].asBool() && e.serialize()["algorithm"].asString() == "soundtouch", name << ": kept with the soundtouch algorithm");
}

static void json_formant()
{
	json_bool_key<Pitch_modifier>("Pitch_modifier", "formant");
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
	Json::Value vel;
	vel["formant"] = true;
	Velocity_modifier h;
	h.deserialize(vel);
	CHECK(!h.serialize().isMember("formant"), "Velocity_modifier has no formant key");
}

template <class Node>
static void json_transients(const char* name, bool pitch_node)
{
	json_bool_key<Node>(name, "transients");
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
	st["phase_lock"] = true;
	Node h;
	h.deserialize(st);
	CHECK(h.serialize()["transients"].asBool() && h.serialize()["phase_lock"].asBool(), name << ": both kept with the soundtouch algorithm");
}

template <class Node>
static void json_link(const char* name, bool pitch_node)
{
	json_bool_key<Node>(name, "link_channels");
	Node node;
	CHECK(node.serialize().size() == (pitch_node ? 1u : 2u), name << ": the default serialisation keeps its key set");
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
}

static bool out_of_range(const Json::Value& v)
{
	Pitch_modifier node;
	try
	{
		node.deserialize(v);
	}
	catch (const infra::Processor::Runtime_error& e)
	{
		return e.detail == "Out of range: formant_shift";
	}
	return false;
}

static void json_formant_shift()
{
	Pitch_modifier node;
	CHECK(!node.serialize().isMember("formant_shift"), "a default node writes no formant_shift");
	for (const Json::Value& s : {Json::Value(4.0), Json::Value(-5.0), Json::Value(3), Json::Value(24), Json::Value(-24.0), Json::Value(0.5)})
	{
		Json::Value v;
		v["formant_shift"] = s;
		Pitch_modifier a;
		a.deserialize(v);
		const Json::Value w = a.serialize();
		CHECK(w.isMember("formant_shift") && w["formant_shift"].isDouble() && w["formant_shift"].asFloat() == s.asFloat(), "a shift is written back");
		Pitch_modifier b;
		b.deserialize(w);
		CHECK(b.serialize()["formant_shift"].asFloat() == s.asFloat(), "round trip");
		a.deserialize(Json::Value());
		CHECK(!a.serialize().isMember("formant_shift"), "a missing key means 0");
	}
	Json::Value zero;
	zero["formant_shift"] = 0.0;
	Pitch_modifier z;
	z.deserialize(zero);
	CHECK(!z.serialize().isMember("formant_shift"), "0 is not written");
	for (const Json::Value& bad : {Json::Value(true), Json::Value("4"), Json::Value(false)})
	{
		Json::Value v;
		v["formant_shift"] = bad;
		CHECK(rejects<Pitch_modifier>(v, "formant_shift"), "a formant_shift that is not a number is rejected");
	}
	for (double far : {24.5, -24.01, 100.0, -1e9})
	{
		Json::Value v;
		v["formant_shift"] = far;
		CHECK(out_of_range(v), "a formant_shift beyond +-24 semitones is out of range: " << far);
	}
	Json::Value all;
	all["pitch"] = 0.0;
	all["formant_shift"] = 4.0;
	all["phase_lock"] = true;
	all["transients"] = true;
	all["formant"] = true;
	Pitch_modifier c;
	c.deserialize(all);
	const Json::Value cw = c.serialize();
	CHECK(cw["formant_shift"].asFloat() == 4.0f && cw["phase_lock"].asBool() && cw["transients"].asBool() && cw["formant"].asBool() && cw["pitch"].asFloat() == 0.0f,
		  "combines with phase_lock, transients and formant");
	Json::Value sz;
	sz["formant_shift"] = -3.0;
	sz["fft_size"] = 2048;
	Pitch_modifier d;
	d.deserialize(sz);
	CHECK(d.serialize()["formant_shift"].asFloat() == -3.0f && d.serialize()["fft_size"].asInt() == 2048 && !d.serialize().isMember("formant"),
		  "combines with fft_size, and does not set formant");
	Json::Value st;
	st["algorithm"] = "soundtouch";
	st["formant_shift"] = 2.0;
	Pitch_modifier e;
	e.deserialize(st);
	CHECK(e.serialize()["formant_shift"].asFloat() == 2.0f && e.serialize()["algorithm"].asString() == "soundtouch", "kept with the soundtouch algorithm");
	Json::Value vm;
	vm["formant_shift"] = "not a number";
	Velocity_modifier vel;
	vel.deserialize(vm);
	CHECK(!vel.serialize().isMember("formant_shift"), "Velocity_modifier has no such key");
}

static const int S = 60000;  // stereo samples of every graph's input

// uniform noise in amp * [-0.5, 0.5), interleaved stereo
static std::vector<float> noise(uint64_t st, float amp)
{
	std::vector<float> x((size_t)S * 2);
	for (auto& v : x)
	{
		st = st * 6364136223846793005ull + 1442695040888963407ull;
		v = amp * (float)((double)(st >> 40) / (double)(1ull << 24) - 0.5);
	}
	return x;
}

// clicks every 9000 samples over quiet independent noise: in the left channel only, or in both
static std::vector<float> clicks(bool both)
{
	std::vector<float> x = noise(777, 0.02f);
	for (int p = 3000; p < S; p += 9000)
	{
		x[(size_t)p * 2] = 0.9f;
		if (both) x[(size_t)p * 2 + 1] = 0.9f;
	}
	return x;
}

static bool dump(const char* path, const std::vector<float>& a, const std::vector<float>& b = {})
{
	FILE* f = std::fopen(path, "wb");
	CHECK(f != nullptr, "open " << path);
	if (!f) return false;
	const bool ok = std::fwrite(a.data(), sizeof(float), a.size(), f) == a.size() && std::fwrite(b.data(), sizeof(float), b.size(), f) == b.size();
	return std::fclose(f) == 0 && ok;
}

using Block_call = std::function<int(nae_ctx*, const nae_sig*, nae_sig*)>;

// source(x) -> Pitch_modifier(v) -> sink through the fiber runner is `want` on the same samples bit for bit (out_len from the plan's) and, where
// `plain` is given, differs from it; returns the graph's output
static std::vector<float> graph_against_block(const std::vector<float>& x, const Json::Value& v, const std::string& label, size_t out_len,
											  const Block_call& want, const char* want_name, const Block_call& plain, const char* plain_name)
{
	Runner r;
	auto src = std::make_shared<Src>();
	src->samples = x;
	auto pitch = std::make_shared<Pitch_modifier>();
	pitch->deserialize(v);
	auto sink = std::make_shared<Sink>();
	r.add_node(1, src); r.add_node(2, pitch); r.add_node(3, sink);
	r.add_link({1, "output", 2, "input"});
	r.add_link({2, "output", 3, "input"});
	const bool ok = r.run();
	CHECK(ok, "source -> pitch(" << label << ") -> sink runs: " << r.get_processor_resources().at(2)->error_text);
	std::vector<float> got;
	if (!ok) return got;
	for (auto& f : sink->frames)
	{
		const Frame_data* d = f->data();
		CHECK(d->format == AV_SAMPLE_FMT_FLT && d->ch_layout.nb_channels == 2, "interleaved stereo f32 out");
		const float* p = reinterpret_cast<const float*>(d->data[0]);
		got.insert(got.end(), p, p + (size_t)d->nb_samples * 2);
	}
	nae_ctx* ctx = nullptr;
	CHECK(nae_ctx_create(0, &ctx) == 0, "context");
	if (!ctx) return got;
	void *d_x = nullptr, *d_o = nullptr;
	CHECK(nae_malloc(ctx, x.size() * sizeof(float), &d_x) == 0 && nae_malloc(ctx, out_len * 2 * sizeof(float), &d_o) == 0, "malloc");
	CHECK(nae_memcpy_h2d(ctx, d_x, x.data(), x.size() * sizeof(float)) == 0, "h2d");
	nae_sig si{d_x, (size_t)S * 2, 1, 2}, so{d_o, out_len * 2, 1, 2};
	std::vector<float> ref(out_len * 2), other(out_len * 2);
	CHECK(want(ctx, &si, &so) == 0, want_name);
	CHECK(nae_memcpy_d2h(ctx, ref.data(), d_o, ref.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	if (plain)
	{
		CHECK(plain(ctx, &si, &so) == 0, plain_name);
		CHECK(nae_memcpy_d2h(ctx, other.data(), d_o, other.size() * sizeof(float)) == 0 && nae_sync(ctx) == 0, "d2h");
	}
	nae_free(ctx, d_x);
	nae_free(ctx, d_o);
	nae_ctx_destroy(ctx);
	CHECK(got.size() == ref.size(), "output length " << got.size() << " vs " << ref.size());
	CHECK(got.size() == ref.size() && std::memcmp(got.data(), ref.data(), ref.size() * sizeof(float)) == 0,
		  "graph output bit-identical to " << want_name);
	if (plain)
		CHECK(got.size() == other.size() && std::memcmp(got.data(), other.data(), ref.size() * sizeof(float)) != 0, "and not " << plain_name);
	return got;
}

// fft_size, phase_lock, formant: the key alone on white noise
static void test_gpu(const std::string& key, const char* out_path)
{
	const bool sizes = key == "fft_size", lock = key == "phase_lock";
	const int N = sizes ? 4096 : 1024;
	const float semis = key == "formant" ? 4.0f : 3.0f;
	const std::vector<float> x = noise(777, 1.0f);
	Json::Value v;
	v["pitch"] = (double)semis;
	v[key] = sizes ? Json::Value(N) : Json::Value(true);
	const double pf = (double)std::pow(2.0f, semis / 12.0f);  // what Pitch_modifier passes
	nae_stretch_plan pl;
	CHECK((lock ? nae_stretch_plan_make(1.0, pf, S, &pl) : nae_stretch_plan_make_n(1.0, pf, N, S, &pl)) == 0, "plan");
	const int lifter = nae_stretch_formant_lifter(48000, N);
	if (key == "formant") CHECK(lifter == 68, "lifter at 48 kHz: " << lifter);
	Block_call want, plain;
	const char* name;
	if (sizes) { name = "the 4096-point block call"; want = [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_n_f32(c, 1.0, pf, 0u, N, si, S, 2, 1, so); }; }
	else if (lock)
	{
		name = "the locked block call";
		want = [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_ex_f32(c, 1.0, pf, NAE_STRETCH_PHASE_LOCK, si, S, 2, 1, so); };
		plain = [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_f32(c, 1.0, pf, si, S, 2, 1, so); };
	}
	else { name = "the formant block call"; want = [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_formant_f32(c, 1.0, pf, 0u, N, lifter, si, S, 2, 1, so); }; }
	const std::vector<float> got = graph_against_block(x, v, sizes ? "+3, fft_size 4096" : lock ? "+3, phase_lock" : "+4, formant", pl.out_len, want, name, plain, "the unlocked one");
	if (out_path && !got.empty()) CHECK(dump(out_path, x, got), "input and output written");
}

// transients, link_channels: the key with the flag word `base` (and the node keys that spell it) against the block call without the key
static void test_gpu_flag(const char* key, unsigned flag, unsigned base, const std::vector<float>& x)
{
	const bool lock = base & NAE_STRETCH_PHASE_LOCK;
	const int N = lock ? 1024 : 2048;
	Json::Value v;
	v["pitch"] = 3.0;
	if (lock) v["phase_lock"] = true;
	else v["fft_size"] = N;
	if (base & NAE_STRETCH_TRANSIENTS) v["transients"] = true;
	v[key] = true;
	const double pf = (double)std::pow(2.0f, 3.0f / 12.0f);  // what Pitch_modifier passes
	nae_stretch_plan pl;
	CHECK(nae_stretch_plan_make_n(1.0, pf, N, S, &pl) == 0, "plan");
	auto call = [=](unsigned flags) { return [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_n_f32(c, 1.0, pf, flags, N, si, S, 2, 1, so); }; };
	const std::string label = std::string("+3, ") + (lock ? "phase_lock" : "fft_size 2048") + (base & NAE_STRETCH_TRANSIENTS ? ", transients, " : ", ") + key;
	graph_against_block(x, v, label, pl.out_len, call(base | flag), "the block call with the key's flag", call(base), "the one without it");
}

static void test_gpu_shift(float semis, float shift, const char* in_path, const char* out_path)
{
	const int N = 1024;
	const std::vector<float> x = noise(4242, 0.5f);
	Json::Value v;
	v["pitch"] = (double)semis;
	v["formant_shift"] = (double)shift;
	const double pf = (double)std::pow(2.0f, semis / 12.0f);  // what Pitch_modifier passes
	const double phi = std::pow(2.0, (double)shift / 12.0);
	const int q = nae_stretch_formant_lifter(48000, N);
	nae_stretch_plan pl;
	CHECK(nae_stretch_plan_make_shift(1.0, pf, phi, q, N, S, &pl) == 0, "plan");
	const std::vector<float> got = graph_against_block(
		x, v, std::to_string(semis) + ", formant_shift " + std::to_string(shift), pl.out_len,
		[=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_formant_shift_f32(c, 1.0, pf, 0u, N, q, phi, si, S, 2, 1, so); },
		"the block call with the shift", [=](nae_ctx* c, const nae_sig* si, nae_sig* so) { return nae_stretch_block_n_f32(c, 1.0, pf, 0u, N, si, S, 2, 1, so); },
		"the call without it");
	if (!got.empty()) CHECK(dump(in_path, x) && dump(out_path, got), "input and output written");
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "", key = argc > 2 ? argv[2] : "";
	const bool lock = argc > 3 && std::string(argv[3]) == "lock";
	if (mode == "json" && key == "fft_size") { json_fft_size<Velocity_modifier>("Velocity_modifier"); json_fft_size<Pitch_modifier>("Pitch_modifier"); }
	else if (mode == "json" && key == "phase_lock") { json_bool_key<Velocity_modifier>("Velocity_modifier", "phase_lock"); json_bool_key<Pitch_modifier>("Pitch_modifier", "phase_lock"); }
	else if (mode == "json" && key == "formant") json_formant();
	else if (mode == "json" && key == "transients") { json_transients<Velocity_modifier>("Velocity_modifier", false); json_transients<Pitch_modifier>("Pitch_modifier", true); }
	else if (mode == "json" && key == "link_channels") { json_link<Velocity_modifier>("Velocity_modifier", false); json_link<Pitch_modifier>("Pitch_modifier", true); }
	else if (mode == "json" && key == "formant_shift") json_formant_shift();
	else if (mode == "gpu" && (key == "fft_size" || key == "phase_lock" || key == "formant")) test_gpu(key, argc > 3 ? argv[3] : nullptr);
	else if (mode == "gpu" && key == "transients") test_gpu_flag("transients", NAE_STRETCH_TRANSIENTS, lock ? NAE_STRETCH_PHASE_LOCK : 0u, clicks(true));
	else if (mode == "gpu" && key == "link_channels")
		test_gpu_flag("link_channels", NAE_STRETCH_LINK_CHANNELS, lock ? NAE_STRETCH_PHASE_LOCK : NAE_STRETCH_TRANSIENTS, clicks(false));
	else if (mode == "gpu" && key == "formant_shift" && argc == 7) test_gpu_shift((float)std::atof(argv[3]), (float)std::atof(argv[4]), argv[5], argv[6]);
	else
	{
		std::cout << "usage: host_pv_node json <key> | gpu fft_size|phase_lock|formant [out.f32] | gpu transients|link_channels [lock] | "
					 "gpu formant_shift <pitch> <shift> <in.f32> <out.f32>\n";
		return 2;
	}
	if (failures) { std::cout << failures << " failure(s)\n"; return 1; }
	std::cout << "HOST PV NODE OK " << mode << " " << key << (lock ? " lock" : "") << "\n";
	return 0;
}
