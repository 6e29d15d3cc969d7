// processor/audio-effects.cpp — the nodes on a block streaming handle: Audio_filter (nae_fir), Audio_reverb (nae_conv), Audio_eq (nae_eq),
// Audio_dynamics (nae_dyn), Audio_sidechain (nae_dynkey, two input pins and a loop of its own), Audio_echo (nae_echo), Audio_modulation (nae_mod), Audio_saturation (nae_sat), Audio_gate (nae_gate), Audio_multiband (nae_mb), Audio_denoise (nae_denoise), Audio_separation (nae_hpss), Audio_limiter (nae_lim) and Audio_dither (nae_dither), and the one loop that feeds such a handle and delivers its frames (run_on_handle);
// and Audio_loudness (nae_loud), whose handle measures and hands out no samples: the node holds them and applies the one gain at the end.
// Both loops stand on node-util.hpp's two ends, take_in and cut_and_push; what is written here is what lies between them.
// A node's parameters are stated once: the members and their defaults in the settings record of audio-<node>.hpp, and here, in front of the
// node, ONE list of fields (node-fields.hpp) with each key, its bounds and whatever rule the plain range does not say.  serialize, deserialize
// and the record's clamp (draw-headless.cpp's draw_content) are one call on that list each.  A new node adds its record, its list, those
// three calls and its process_payload; a rule between two fields (the filter's taps against its frame size) is written by hand next to the calls.
#include "audio-filter.hpp"
#include "audio-reverb.hpp"
#include "audio-eq.hpp"
#include "audio-dynamics.hpp"
#include "audio-sidechain.hpp"
#include "audio-echo.hpp"
#include "audio-modulation.hpp"
#include "audio-saturation.hpp"
#include "audio-gate.hpp"
#include "audio-limiter.hpp"
#include "audio-dither.hpp"
#include "audio-multiband.hpp"
#include "audio-denoise.hpp"
#include "audio-separation.hpp"
#include "audio-loudness.hpp"
#include "node-fields.hpp"
#include "nae_dsp_spec.h"

#include <algorithm>
#include <cmath>
#include <optional>
#include <type_traits>

namespace processor
{
	using namespace detail;

	// What the nodes on a streaming handle share (the filter, the reverb, the equalizer, the dynamics node): frames are put as they come, in
	// batches; everything the handle has ready leaves as frames of the input's sizes, pts and time base; the flush at the end of the stream
	// releases the rest, and what is left behind the last frame owed is dropped.  `create` makes the handle from the first frame (its sample
	// rate) and the channel count, or throws.  The first `to_discard` frames of the handle's output are dropped (a linear-phase filter's group
	// delay); `noun` is the node's word for itself in the "Channel count changed" error; ops.name is the prefix of the handle's entries.
	// run_on_handle_held is the loop itself, between the intake (take_in) and the cutting of the output (cut_and_push): hold(first frame) says
	// how many samples must have arrived before the handle is made (the noise reduction learns from a stretch of its input).  Until then, or
	// until the stream ends, the frames wait; create(ctx, first frame, ch, samples, total) then sees everything held, on the device as
	// interleaved f32, and all of it is the handle's first put.
	template <class Handle>
	struct Handle_ops
	{
		const char* name;
		int (*put)(Handle*, const float*, size_t);
		int (*flush)(Handle*);
		size_t (*available)(Handle*);
		int (*receive)(Handle*, float*, size_t, size_t*);
		int (*destroy)(Handle*);
	};

	// The way out of a node on a handle: everything the handle has ready comes down behind ONE wait and leaves as frames of the shapes owed
	// (cut_and_push).  The first to_discard frames of the handle's output are dropped.
	struct Handle_output
	{
		gpu::Device_buffer d_out;
		gpu::Pinned_buffer h_out;
		std::vector<float> ready;     // processed samples behind the discarded ones, interleaved, not yet cut into frames
		size_t ready_pos = 0;         // frames of `ready` already delivered
		size_t to_discard = 0;

		template <class Handle>
		void deliver(Handle* h, const Handle_ops<Handle>& ops, int ch, std::deque<Shape>& shapes, const Output_streams& output_stream,
					 const std::atomic<bool>& stop_token)
		{
			nae_ctx* ctx = gpu::context();
			const size_t avail = ops.available(h);
			if (avail == 0) { gpu::wait(stop_token); return; }
			float* dev = static_cast<float*>(d_out.reserve(avail * ch * sizeof(float)));
			float* host = static_cast<float*>(h_out.reserve(avail * ch * sizeof(float)));
			size_t got = 0;
			const int rc = ops.receive(h, dev, avail, &got);
			if (rc != NAE_OK) gpu::check(rc, (std::string(ops.name) + "_receive").c_str());
			gpu::check(nae_memcpy_d2h(ctx, host, dev, got * ch * sizeof(float)), "d2h");
			gpu::wait(stop_token);
			ready.erase(ready.begin(), ready.begin() + ready_pos * ch);
			const size_t skip = std::min(to_discard, got);
			to_discard -= skip;
			ready.insert(ready.end(), host + skip * ch, host + got * ch);
			ready_pos = cut_and_push(shapes, ready.data(), ready.size() / ch, ch, output_stream, stop_token);
		}
	};

	template <class Handle, class Hold, class Create>
	static void run_on_handle_held(
		Audio_stream& input_stream, const Output_streams& output_stream, const std::atomic<bool>& stop_token,
		const std::type_identity_t<Handle_ops<Handle>>& ops, const char* noun, size_t to_discard, const Hold& hold, const Create& create
	)
	{
		nae_ctx* ctx = gpu::context();
		Handle* h = nullptr;
		struct Guard { Handle*& h; int (*destroy)(Handle*); ~Guard() { if (h) destroy(h); } } guard{h, ops.destroy};
		gpu::Device_buffer d_raw, d_f32;
		gpu::Pinned_buffer h_raw;
		Intake in;
		Handle_output out;
		out.to_discard = to_discard;

		// a failed GPU call is reported by its entry's name (ops.name + suffix), put together only when it failed
		const auto check = [&](int rc, const char* suffix) { if (rc != NAE_OK) gpu::check(rc, (std::string(ops.name) + suffix).c_str()); };

		const auto deliver = [&]() { out.deliver(h, ops, in.ch, in.shapes, output_stream, stop_token); };

		while (!stop_token)
		{
			if (!take_in(in, input_stream, noun, hold)) continue;
			if (!in.pending.empty() && (h != nullptr || in.pending_samples >= in.need || in.at_end))
			{
				size_t total = 0;
				float* samples = upload_as_f32(in.pending, h_raw, d_raw, d_f32, &total);
				if (h == nullptr) h = create(ctx, in.pending.front()->data(), in.ch, samples, total);
				check(ops.put(h, samples, total), "_put");
				in.pending.clear();
				in.pending_samples = 0;
				deliver();
			}
			if (in.at_end)
			{
				if (h != nullptr)
				{
					// what the handle still holds comes out with the flush: every frame still owed is complete
					check(ops.flush(h), "_flush");
					deliver();
				}
				break;
			}
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// a handle made from the first frame alone: nothing is held
	template <class Handle, class Create>
	static void run_on_handle(
		Audio_stream& input_stream, const Output_streams& output_stream, const std::atomic<bool>& stop_token,
		const std::type_identity_t<Handle_ops<Handle>>& ops, const char* noun, size_t to_discard, const Create& create
	)
	{
		run_on_handle_held<Handle>(
			input_stream, output_stream, stop_token, ops, noun, to_discard, [](const Frame_data*) { return (size_t)0; },
			[&](nae_ctx* ctx, const Frame_data* frame, int ch, const float*, size_t) { return create(ctx, frame, ch); }
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_filter
	namespace
	{
		const char* const kind_names[] = {"lowpass", "highpass", "bandpass", "bandstop"};
		// a corner lies inside (0, 1e9), both ends open; the widgets keep it from 1 Hz up
		constexpr Rule<float> corner{[](double hz, double lo, double hi) { return hz > lo && hz < hi; }, above_lo_unbounded<1.0f>.keep};
		// an odd tap count; clamp makes an even one the next odd one
		constexpr Rule<int> odd{[](int n, int, int) { return (n & 1) == 1; }, [](int n, int lo, int hi) { return std::clamp(n, lo, hi) | 1; }};
		// one of the library's frame sizes (512, 1024, 2048, 4096), 0 when absent: the library's pick
		constexpr Rule<int> frame_size{[](int n, int, int) { return nae_fir_pick_n_fft(n / 2 + 1) == n; }, as_it_is<int>};
		constexpr Number filter_fft_size{"fft_size", &Filter_settings::fft_size, 0, 1, 4096, frame_size};
		constexpr std::tuple filter_fields{
			Choice{"kind", &Filter_settings::kind, kind_names},
			Number{"f_lo", &Filter_settings::f_lo, Filter_settings::default_f_lo, 0.0, 1e9, corner},
			Number{"f_hi", &Filter_settings::f_hi, Filter_settings::default_f_hi, 0.0, 1e9, corner},
			Number{"taps", &Filter_settings::taps, Filter_settings::default_taps, 1, Filter_settings::max_taps, odd},
			filter_fft_size,
		};
	}

	infra::Processor::Info Audio_filter::get_processor_info()
	{
		return {"audio_filter", "Audio Filter", false, [] { return std::unique_ptr<infra::Processor>(new Audio_filter); },
				"Linear-phase FIR low-pass / high-pass / band-pass / band-stop by FFT fast convolution (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_filter::get_pin_attributes() const { return io_pins(); }

	Json::Value Audio_filter::serialize() const { return to_json(*this, filter_fields); }

	void Audio_filter::deserialize(const Json::Value& value)
	{
		const Filter_settings read = from_json<Filter_settings>(value, "Audio_filter", filter_fields);
		// a frame size that was given must hold the taps
		if (read.fft_size != 0 && read.taps > read.fft_size / 2 + 1) throw wrong_field("Audio_filter", filter_fft_size.key);
		Filter_settings::operator=(read);
	}

	void Filter_settings::clamp() { detail::clamp(*this, filter_fields); }

	void Audio_filter::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Filter");
		// the group delay is dropped in front; the tail makes up for it: (L - 1) / 2 of the L - 1 flushed frames complete the frames still owed
		run_on_handle<nae_fir>(
			io.input, io.output, stop_token,
			{"nae_fir", nae_fir_put, nae_fir_flush, nae_fir_available, nae_fir_receive, nae_fir_destroy}, "filter", (size_t)(taps - 1) / 2,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				std::vector<float> h((size_t)taps);
				if (nae_fir_design((int)kind, frame->sample_rate, f_lo, f_hi, taps, h.data()) != NAE_OK)
					throw Runtime_error(
						"Invalid filter frequencies", "The filter's corner frequencies must lie below half of the sample rate, the lower below the upper.",
						infra::fmt("f_lo %g Hz, f_hi %g Hz at %d Hz", (double)f_lo, (double)f_hi, frame->sample_rate)
					);
				nae_fir* fir = nullptr;
				gpu::check(nae_fir_create(ctx, h.data(), taps, fft_size, ch, &fir), "nae_fir_create");
				return fir;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_reverb
	infra::Processor::Info Audio_reverb::get_processor_info()
	{
		return {"audio_reverb", "Audio Reverb", false, [] { return std::unique_ptr<infra::Processor>(new Audio_reverb); },
				"Convolution reverb with a designed, per-channel decaying-noise response by partitioned FFT convolution (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_reverb::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		// an exact integer below 2^53, written as a double; not clamped
		struct Seed
		{
			const char* key;

			void write(const Reverb_settings& r, Json::Value& value) const { if (r.seed != Reverb_settings::default_seed) value[key] = (double)r.seed; }
			void read(Reverb_settings& r, const Json::Value& value, const char* node_name) const
			{
				r.seed = Reverb_settings::default_seed;
				if (!value.isMember(key)) return;
				// compared as a double with the range first: a number outside the integer range is never converted
				const Json::Value& v = value[key];
				if (!v.isDouble() || !(v.asDouble() >= 0.0 && v.asDouble() < 9007199254740992.0) || v.asDouble() != (double)(uint64_t)v.asDouble()) throw wrong_field(node_name, key);
				r.seed = (uint64_t)v.asDouble();
			}
			void keep(Reverb_settings&) const {}
		};
		constexpr std::tuple reverb_fields{
			Number{"rt60", &Reverb_settings::rt60, Reverb_settings::default_rt60, 0.1, 5.0},
			Number{"predelay_ms", &Reverb_settings::predelay_ms, Reverb_settings::default_predelay_ms, 0.0, 200.0},
			Number{"wet", &Reverb_settings::wet, Reverb_settings::default_wet, 0.0, 1.0},
			Number{"dry", &Reverb_settings::dry, Reverb_settings::default_dry, 0.0, 1.0},
			Seed{"seed"},
			Number{"fft_size", &Reverb_settings::fft_size, 0, 1, 4096, frame_size},   // the filter's sizes
		};
	}

	Json::Value Audio_reverb::serialize() const { return to_json(*this, reverb_fields); }
	void Audio_reverb::deserialize(const Json::Value& value) { Reverb_settings::operator=(from_json<Reverb_settings>(value, "Audio_reverb", reverb_fields)); }
	void Reverb_settings::clamp() { detail::clamp(*this, reverb_fields); }

	void Audio_reverb::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Reverb");
		// the last partial block comes out with the flush; the frames still owed are cut from it and the tail behind them is dropped
		run_on_handle<nae_conv>(
			io.input, io.output, stop_token,
			{"nae_conv", nae_conv_put, nae_conv_flush, nae_conv_available, nae_conv_receive, nae_conv_destroy}, "reverb", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				const int n_taps = nae_conv_reverb_taps(frame->sample_rate, rt60, predelay_ms / 1000.0);
				if (n_taps < 1 || nae_conv_pick_n_fft(n_taps) == 0)   // the library's limits: 0 beyond them
					throw Runtime_error(
						"Reverb response too long", "The decay time and the pre-delay give a response longer than the convolution supports at this sample rate.",
						infra::fmt("rt60 %g s, pre-delay %g ms at %d Hz: %d taps", rt60, predelay_ms, frame->sample_rate, n_taps)
					);
				std::vector<float> h((size_t)n_taps * ch);
				for (int c = 0; c < ch; c++)
					if (nae_conv_design_reverb(frame->sample_rate, rt60, predelay_ms / 1000.0, dry, wet, seed + (uint64_t)c, n_taps, h.data() + (size_t)c * n_taps) != NAE_OK)
						throw Runtime_error("Invalid reverb parameters", "The reverb's response could not be designed.",
											infra::fmt("rt60 %g s, pre-delay %g ms at %d Hz", rt60, predelay_ms, frame->sample_rate));
				nae_conv* conv = nullptr;
				gpu::check(nae_conv_create(ctx, h.data(), n_taps, ch, fft_size, ch, &conv), "nae_conv_create");
				return conv;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_eq
	infra::Processor::Info Audio_eq::get_processor_info()
	{
		return {"audio_eq", "Audio Equalizer", false, [] { return std::unique_ptr<infra::Processor>(new Audio_eq); },
				"Parametric equalizer: up to 16 peaking, shelving, low-pass, high-pass and notch bands as a biquad cascade in double (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_eq::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const eq_kind_names[] = {"peak", "lowshelf", "highshelf", "lowpass", "highpass", "notch"};
		constexpr std::tuple band_fields{
			Choice{"kind", &Audio_eq::Band::kind, eq_kind_names},
			Number{"freq", &Audio_eq::Band::freq, Audio_eq::Band::default_freq, 0.0, 1e9, above_lo_unbounded<1.0>},
			Number{"gain_db", &Audio_eq::Band::gain_db, Audio_eq::Band::default_gain_db, -24.0, 24.0},
			Number{"q", &Audio_eq::Band::q, Audio_eq::Band::default_q, 0.1, 40.0},
		};
	}

	void Audio_eq::Band::clamp() { detail::clamp(*this, band_fields); }

	// a list of bands in audio_eq's format, which audio_sidechain's "key_filter" has too: the defaults are not written
	static Json::Value bands_to_json(const std::vector<Audio_eq::Band>& bands)
	{
		Json::Value list(Json::arrayValue);
		for (const Audio_eq::Band& b : bands) list.append(to_json(b, band_fields));
		return list;
	}

	// value[key], if there, as at most max_bands bands; the list's own faults are "Wrong field: <key>", a band's "Wrong field: <its key>"
	static std::vector<Audio_eq::Band> bands_from_json(const Json::Value& value, const char* node_name, const char* key, size_t max_bands)
	{
		std::vector<Audio_eq::Band> read;
		if (!value.isMember(key)) return read;
		const Json::Value& list = value[key];
		if (!list.isArray() || list.size() > max_bands) throw wrong_field(node_name, key);
		for (int i = 0; i < (int)list.size(); i++)
		{
			const Json::Value& v = list[i];
			if (v.isArray() || v.isDouble() || v.isBool() || v.isString()) throw wrong_field(node_name, key);   // an object, possibly without a key
			read.push_back(from_json<Audio_eq::Band>(v, node_name, band_fields));
		}
		return read;
	}

	// the bands' sections at the stream's sample rate (nae_eq_design); a band at or above Nyquist is the user's error
	static std::vector<double> design_bands(const std::vector<Audio_eq::Band>& bands, int sample_rate)
	{
		std::vector<double> coef(bands.size() * 5);
		for (size_t i = 0; i < bands.size(); i++)
			if (nae_eq_design((int)bands[i].kind, sample_rate, bands[i].freq, bands[i].gain_db, bands[i].q, coef.data() + 5 * i) != NAE_OK)
				throw infra::Processor::Runtime_error("Invalid equalizer band", "A band's frequency must lie below half the stream's sample rate.",
									infra::fmt("band %d: %g Hz at %d Hz", (int)i, bands[i].freq, sample_rate));
		return coef;
	}

	Json::Value Audio_eq::serialize() const
	{
		Json::Value value;
		if (!bands.empty()) value["bands"] = bands_to_json(bands);
		return value;
	}

	// everything is read and checked first: a rejected value leaves the node as it was
	void Audio_eq::deserialize(const Json::Value& value) { bands = bands_from_json(value, "Audio_eq", "bands", max_bands); }

	void Audio_eq::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Equalizer");
		if (bands.empty())
		{
			pass_through(io.input, io.output, stop_token);
			return;
		}
		run_on_handle<nae_eq>(
			io.input, io.output, stop_token, {"nae_eq", nae_eq_put, nae_eq_flush, nae_eq_available, nae_eq_receive, nae_eq_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				const std::vector<double> coef = design_bands(bands, frame->sample_rate);
				nae_eq* eq = nullptr;
				gpu::check(nae_eq_create(ctx, coef.data(), (int)bands.size(), ch, &eq), "nae_eq_create");
				return eq;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_dynamics
	infra::Processor::Info Audio_dynamics::get_processor_info()
	{
		return {"audio_dynamics", "Audio Dynamics", false, [] { return std::unique_ptr<infra::Processor>(new Audio_dynamics); },
				"Compressor / look-ahead limiter in the dB domain: threshold, ratio, soft knee, attack, release, make-up gain (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_dynamics::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const dynamics_mode_names[] = {"compressor", "limiter"};
		constexpr std::tuple dynamics_fields{
			Choice{"mode", &Dynamics_settings::mode, dynamics_mode_names},
			Number{"threshold_db", &Dynamics_settings::threshold_db, Dynamics_settings::default_threshold_db, NAE_DYN_MIN_THRESHOLD_DB, NAE_DYN_MAX_THRESHOLD_DB},
			Number{"ratio", &Dynamics_settings::ratio, Dynamics_settings::default_ratio, 1.0, 100.0},
			Number{"knee_db", &Dynamics_settings::knee_db, Dynamics_settings::default_knee_db, 0.0, NAE_DYN_MAX_KNEE_DB},
			Number{"attack_ms", &Dynamics_settings::attack_ms, Dynamics_settings::default_attack_ms, 0.0, 500.0},
			Number{"release_ms", &Dynamics_settings::release_ms, Dynamics_settings::default_release_ms, 1.0, 5000.0},
			Number{"lookahead_ms", &Dynamics_settings::lookahead_ms, Dynamics_settings::default_lookahead_ms, 0.0, 20.0},
			Number{"makeup_db", &Dynamics_settings::makeup_db, Dynamics_settings::default_makeup_db, -NAE_DYN_MAX_MAKEUP_DB, NAE_DYN_MAX_MAKEUP_DB},
			Flag{"link_channels", &Dynamics_settings::link_channels, true},
		};
	}

	void Dynamics_settings::clamp() { detail::clamp(*this, dynamics_fields); }

	// the settings as the library's parameters at the stream's sample rate (nae_dyn_design); a look-ahead too long for that rate is the user's error
	static nae_dyn_params design_dynamics(const Dynamics_settings& s, int sample_rate)
	{
		nae_dyn_params params;
		const int rc = nae_dyn_design(sample_rate, s.threshold_db, s.mode == Dynamics_settings::Mode::Limiter ? INFINITY : s.ratio, s.knee_db,
									  s.attack_ms / 1000.0, s.release_ms / 1000.0, s.lookahead_ms / 1000.0, s.makeup_db, s.link_channels ? 1 : 0, &params);
		if (rc == NAE_ERR_UNSUPPORTED)
			throw infra::Processor::Runtime_error("Look-ahead too long", "The look-ahead must not exceed 1024 samples at the stream's sample rate.",
								infra::fmt("lookahead %g ms at %d Hz", s.lookahead_ms, sample_rate));
		if (rc != NAE_OK)
			throw infra::Processor::Runtime_error("Invalid dynamics parameters", "A parameter of the dynamics node lies outside its range.",
								infra::fmt("nae_dyn_design at %d Hz: code %d", sample_rate, rc));
		return params;
	}

	Json::Value Audio_dynamics::serialize() const { return to_json(*this, dynamics_fields); }
	void Audio_dynamics::deserialize(const Json::Value& value) { Dynamics_settings::operator=(from_json<Dynamics_settings>(value, "Audio_dynamics", dynamics_fields)); }

	void Audio_dynamics::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Dynamics");
		run_on_handle<nae_dyn>(
			io.input, io.output, stop_token, {"nae_dyn", nae_dyn_put, nae_dyn_flush, nae_dyn_available, nae_dyn_receive, nae_dyn_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				const nae_dyn_params params = design_dynamics(*this, frame->sample_rate);
				nae_dyn* dyn = nullptr;
				gpu::check(nae_dyn_create(ctx, &params, ch, &dyn), "nae_dyn_create");
				return dyn;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_sidechain
	infra::Processor::Info Audio_sidechain::get_processor_info()
	{
		return {"audio_sidechain", "Audio Side-chain Dynamics", false, [] { return std::unique_ptr<infra::Processor>(new Audio_sidechain); },
				"Compressor / limiter whose detector listens to a key input, or to the signal through a filter: ducking, de-essing (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_sidechain::get_pin_attributes() const
	{
		std::vector<infra::Processor::Pin_attribute> pins = io_pins();
		pins.push_back({"key", "Key", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }});
		return pins;
	}

	Json::Value Audio_sidechain::serialize() const
	{
		Json::Value value = to_json(dynamics, dynamics_fields);
		if (!key_filter.empty()) value["key_filter"] = bands_to_json(key_filter);
		return value;
	}

	void Audio_sidechain::deserialize(const Json::Value& value)
	{
		// everything is read and checked first: a rejected value leaves the node as it was
		const Dynamics_settings d = from_json<Dynamics_settings>(value, "Audio_sidechain", dynamics_fields);
		std::vector<Audio_eq::Band> bands = bands_from_json(value, "Audio_sidechain", "key_filter", max_bands);
		dynamics = d;
		key_filter = std::move(bands);
	}

	namespace
	{
		// One pin of the side-chain node: every frame that waits is taken at once and its samples are kept as interleaved f32 on the host, from
		// `base` (the stream's sample index of samples[0]) on; `total` samples have arrived.  Packed float frames (and mono planar ones) already
		// are those samples; the others are converted on the device (upload_as_f32) and come back from there, waited for.
		struct Pin_intake
		{
			int ch = 0, sample_rate = 0;
			double t0 = 0.0;               // the first frame's pts in seconds
			bool started = false, ended = false;
			std::vector<float> samples;
			size_t base = 0, total = 0;
			std::deque<Shape> shapes;      // of every frame taken (the input pin's are the output's)
			gpu::Device_buffer d_raw, d_f32;
			gpu::Pinned_buffer h_raw, h_f32;

			// -> whether anything came
			bool take(Audio_stream& stream, const char* what, const std::atomic<bool>& stop_token)
			{
				std::vector<Frame_ptr> batch;
				while (true)
				{
					const auto pop_result = stream.try_pop();
					if (!pop_result.has_value())
					{
						ended = stream.eof();
						break;
					}
					batch.push_back(pop_result.value());
				}
				if (batch.empty()) return false;
				const Frame_data* first = batch.front()->data();
				if (!started)
				{
					started = true;
					ch = first->ch_layout.nb_channels;
					sample_rate = first->sample_rate;
					t0 = (double)first->pts * (double)first->time_base.num / (double)first->time_base.den;
					if (ch != 1 && ch != 2)
						throw infra::Processor::Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels on %s", ch, what));
				}
				bool wire = true;
				for (const auto& f : batch)
				{
					const Frame_data* d = f->data();
					if (d->ch_layout.nb_channels != ch || d->sample_rate != sample_rate)
						throw infra::Processor::Runtime_error("Stream format changed", "The node runs streams of a fixed channel count and sample rate.",
															  infra::fmt("Got %d channels at %d Hz after %d at %d Hz on %s", d->ch_layout.nb_channels, d->sample_rate, ch, sample_rate, what));
					shapes.push_back({d->nb_samples, d->sample_rate, d->pts, d->time_base});
					wire = wire && (d->format == AV_SAMPLE_FMT_FLT || (d->format == AV_SAMPLE_FMT_FLTP && ch == 1));
				}
				if (wire)
					for (const auto& f : batch)
					{
						const float* data = reinterpret_cast<const float*>(f->data()->data[0]);
						samples.insert(samples.end(), data, data + (size_t)f->data()->nb_samples * ch);
						total += (size_t)f->data()->nb_samples;
					}
				else
				{
					size_t n = 0;
					float* dev = upload_as_f32(batch, h_raw, d_raw, d_f32, &n);
					float* host = static_cast<float*>(h_f32.reserve(n * ch * sizeof(float)));
					gpu::check(nae_memcpy_d2h(gpu::context(), host, dev, n * ch * sizeof(float)), "d2h");
					gpu::wait(stop_token);
					samples.insert(samples.end(), host, host + n * ch);
					total += n;
				}
				return true;
			}

			// forget the samples below stream index `upto`
			void drop(size_t upto)
			{
				if (upto <= base) return;
				samples.erase(samples.begin(), samples.begin() + std::min(samples.size(), (upto - base) * (size_t)ch));
				base = upto;
			}
		};
	}

	void Audio_sidechain::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Side-chain Dynamics");
		const auto key_item = infra::get_input_item<Audio_stream>(input, "key");   // not connected: the signal is its own key
		nae_ctx* ctx = gpu::context();
		const Handle_ops<nae_dynkey> ops{"nae_dynkey", nae_dynkey_put, nae_dynkey_flush, nae_dynkey_available, nae_dynkey_receive, nae_dynkey_destroy};
		nae_dynkey* h = nullptr;
		struct Guard { nae_dynkey*& h; ~Guard() { if (h) nae_dynkey_destroy(h); } } guard{h};
		Pin_intake in, key;
		Handle_output out;
		std::vector<float> frames;   // a put: the signal's channels, then the key's, frame by frame
		long long o = 0;             // the key sample for input sample n is key[n - o]
		int key_ch = 0;
		size_t put = 0;              // input samples put
		if (!key_item.has_value()) key.ended = true;

		while (!stop_token)
		{
			bool moved = in.take(io.input, "the input", stop_token);
			if (key_item.has_value() && key.take(key_item.value().get(), "the key", stop_token)) moved = true;
			if (h == nullptr && in.started && (key.started || key.ended))
			{
				// the first frames: the key is lined up once, and the handle is made for the input's channels and the key's
				if (key.started)
				{
					if (key.sample_rate != in.sample_rate)
						throw Runtime_error("Key sample rate differs", "The key must have the input's sample rate.",
											infra::fmt("key %d Hz, input %d Hz", key.sample_rate, in.sample_rate));
					if (key.ch != 1 && key.ch != in.ch)
						throw Runtime_error("Key channel count", "The key must be mono or have the input's channel count.",
											infra::fmt("key %d channels, input %d", key.ch, in.ch));
					o = std::llround((key.t0 - in.t0) * (double)in.sample_rate);
				}
				// a key pin that ended without a frame keys with silence
				key_ch = key_item.has_value() ? (key.started ? key.ch : 1) : 0;
				nae_dynkey_params params{};
				params.dyn = design_dynamics(dynamics, in.sample_rate);
				params.key_ch = key_ch;
				params.n_sections = (int)key_filter.size();
				const std::vector<double> coef = design_bands(key_filter, in.sample_rate);
				std::copy(coef.begin(), coef.end(), &params.coef[0][0]);
				gpu::check(nae_dynkey_create(ctx, &params, in.ch, &h), "nae_dynkey_create");
			}
			if (h != nullptr)
			{
				// an input sample is put when its key sample has arrived or the key stream has ended
				size_t upto = in.total;
				if (key_ch && !key.ended) upto = (size_t)std::clamp<long long>((long long)key.total + o, 0, (long long)in.total);
				if (upto > put)
				{
					const size_t n = upto - put, w = (size_t)(in.ch + key_ch);
					frames.assign(n * w, 0.0f);   // zero outside what the key stream delivered
					for (size_t i = 0; i < n; i++)
					{
						for (int c = 0; c < in.ch; c++) frames[i * w + c] = in.samples[(put + i - in.base) * in.ch + c];
						const long long j = (long long)(put + i) - o;
						if (key_ch && j >= 0 && (size_t)j < key.total)
							for (int c = 0; c < key_ch; c++) frames[i * w + in.ch + c] = key.samples[((size_t)j - key.base) * key_ch + c];
					}
					gpu::check(nae_dynkey_put_host(h, frames.data(), n), "nae_dynkey_put_host");
					put = upto;
					in.drop(put);
					if (key_ch) key.drop((size_t)std::max<long long>((long long)put - o, 0));
					out.deliver(h, ops, in.ch, in.shapes, io.output, stop_token);
					moved = true;
				}
				if (in.ended && put == in.total)
				{
					gpu::check(nae_dynkey_flush(h), "nae_dynkey_flush");
					out.deliver(h, ops, in.ch, in.shapes, io.output, stop_token);
					break;
				}
			}
			else if (in.ended && !in.started) break;   // an input without a frame
			if (!moved) nae_fiber::this_fiber::yield();
		}
		for (auto& stream : io.output) stream->set_eof();
	}

	// ------------------------------------------------------------------------------------------ Audio_echo
	infra::Processor::Info Audio_echo::get_processor_info()
	{
		return {"audio_echo", "Audio Echo", false, [] { return std::unique_ptr<infra::Processor>(new Audio_echo); },
				"Echo: a feedback delay with damped repeats, per-channel delay times and ping-pong between the channels (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_echo::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		// a delay has no range of its own but its sign: what it may be depends on the stream's sample rate (process_payload)
		constexpr std::tuple echo_fields{
			Number{"delay_ms", &Echo_settings::delay_ms, Echo_settings::default_delay_ms, 0.0, 1e9, above_lo<1.0>},
			Optional_real{"delay_ms_right", &Echo_settings::delay_ms_right, 0.0, 1e9, above_lo<1.0>},
			Number{"feedback", &Echo_settings::feedback, Echo_settings::default_feedback, 0.0, 0.95},
			Flag{"ping_pong", &Echo_settings::ping_pong, false},
			Number{"damp_hz", &Echo_settings::damp_hz, Echo_settings::default_damp_hz, 0.0, 20000.0, none_or_from<200.0>},
			Number{"lowcut_hz", &Echo_settings::lowcut_hz, Echo_settings::default_lowcut_hz, 0.0, 2000.0, none_or_from<20.0>},
			Number{"wet", &Echo_settings::wet, Echo_settings::default_wet, 0.0, 1.0},
			Number{"dry", &Echo_settings::dry, Echo_settings::default_dry, 0.0, 1.0},
		};
	}

	Json::Value Audio_echo::serialize() const { return to_json(*this, echo_fields); }
	void Audio_echo::deserialize(const Json::Value& value) { Echo_settings::operator=(from_json<Echo_settings>(value, "Audio_echo", echo_fields)); }
	void Echo_settings::clamp() { detail::clamp(*this, echo_fields); }

	void Audio_echo::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Echo");
		run_on_handle<nae_echo>(
			io.input, io.output, stop_token, {"nae_echo", nae_echo_put, nae_echo_flush, nae_echo_available, nae_echo_receive, nae_echo_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				// the delays at the stream's sample rate: the library runs 1024 ... 1048576 samples
				const double right_ms = delay_ms_right.value_or(delay_ms);
				for (const double ms : {delay_ms, right_ms})
				{
					const double samples = ms / 1000.0 * frame->sample_rate;
					const long long n = std::llround(std::min(samples, 1e12));
					if (n < NAE_ECHO_MIN_DELAY || n > NAE_ECHO_MAX_DELAY)
						throw Runtime_error("Echo delay out of range", "The delay must be 1024 to 1048576 samples at the stream's sample rate.",
											infra::fmt("delay %g ms at %d Hz: %g samples", ms, frame->sample_rate, samples));
				}
				nae_echo_params params;
				if (nae_echo_design(frame->sample_rate, delay_ms / 1000.0, right_ms / 1000.0, feedback, damp_hz, lowcut_hz, wet, dry, ping_pong ? 1 : 0, &params) != NAE_OK)
					throw Runtime_error("Invalid echo parameters", "The loop filter's corner frequencies must lie below half the stream's sample rate.",
										infra::fmt("damp %g Hz, low cut %g Hz at %d Hz", damp_hz, lowcut_hz, frame->sample_rate));
				nae_echo* echo = nullptr;
				gpu::check(nae_echo_create(ctx, &params, ch, &echo), "nae_echo_create");
				return echo;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_modulation
	infra::Processor::Info Audio_modulation::get_processor_info()
	{
		return {"audio_modulation", "Audio Modulation", false, [] { return std::unique_ptr<infra::Processor>(new Audio_modulation); },
				"Chorus, flanger and vibrato: a short delay swept by an LFO, up to four voices, feedback and stereo spread (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_modulation::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const shape_names[] = {"sine", "triangle"};
		// a delay has no range of its own but its sign: what it may be depends on the stream's sample rate (process_payload)
		constexpr std::tuple modulation_fields{
			Number{"rate_hz", &Modulation_settings::rate_hz, Modulation_settings::default_rate_hz, 0.0, 20.0},
			Number{"delay_ms", &Modulation_settings::delay_ms, Modulation_settings::default_delay_ms, 0.0, 1e9, above_lo<0.05>},
			Number{"depth_ms", &Modulation_settings::depth_ms, Modulation_settings::default_depth_ms, 0.0, 1e9},
			Number{"feedback", &Modulation_settings::feedback, Modulation_settings::default_feedback, -0.95, 0.95},
			Number{"voices", &Modulation_settings::voices, Modulation_settings::default_voices, 1, NAE_MOD_MAX_VOICES},
			Number{"spread", &Modulation_settings::spread, Modulation_settings::default_spread, 0.0, 1.0},
			Choice{"shape", &Modulation_settings::shape, shape_names},
			Number{"wet", &Modulation_settings::wet, Modulation_settings::default_wet, 0.0, 1.0},
			Number{"dry", &Modulation_settings::dry, Modulation_settings::default_dry, 0.0, 1.0},
		};
	}

	Json::Value Audio_modulation::serialize() const { return to_json(*this, modulation_fields); }
	void Audio_modulation::deserialize(const Json::Value& value) { Modulation_settings::operator=(from_json<Modulation_settings>(value, "Audio_modulation", modulation_fields)); }
	void Modulation_settings::clamp() { detail::clamp(*this, modulation_fields); }

	void Audio_modulation::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Modulation");
		run_on_handle<nae_mod>(
			io.input, io.output, stop_token, {"nae_mod", nae_mod_put, nae_mod_flush, nae_mod_available, nae_mod_receive, nae_mod_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				// the sweep at the stream's sample rate: the library runs 2 ... 3070 samples, and the design is the one statement of that
				nae_mod_params params;
				if (nae_mod_design(frame->sample_rate, rate_hz, delay_ms, depth_ms, feedback, voices, spread, shape == Shape::Triangle ? NAE_MOD_TRIANGLE : NAE_MOD_SINE,
								   wet, dry, &params) != NAE_OK)
					throw Runtime_error("Modulation delay out of range", "The delay less the depth must be at least 2 samples, and the delay plus the depth at most 3070 samples, at the stream's sample rate.",
										infra::fmt("delay %g ms, depth %g ms at %d Hz: %g to %g samples", delay_ms, depth_ms, frame->sample_rate,
												   (delay_ms - depth_ms) * 1e-3 * frame->sample_rate, (delay_ms + depth_ms) * 1e-3 * frame->sample_rate));
				nae_mod* mod = nullptr;
				gpu::check(nae_mod_create(ctx, &params, ch, &mod), "nae_mod_create");
				return mod;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_saturation
	infra::Processor::Info Audio_saturation::get_processor_info()
	{
		return {"audio_saturation", "Audio Saturation", false, [] { return std::unique_ptr<infra::Processor>(new Audio_saturation); },
				"Drive, saturation and clipping: a soft or hard curve run oversampled so its harmonics do not alias (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_saturation::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const curve_names[] = {"soft", "hard"};
		// a factor the library has: 1, 2, 4 ... NAE_SAT_MAX_OS; clamp rounds down to one of them
		constexpr Rule<int> power_of_two{
			[](int os, int, int) { return nae_sat_latency(os) >= 0; },
			[](int os, int lo, int hi) { while (hi > lo && hi > os) hi /= 2; return hi; }};
		constexpr std::tuple saturation_fields{
			Number{"drive_db", &Saturation_settings::drive_db, Saturation_settings::default_drive_db, 0.0, 48.0},
			Choice{"curve", &Saturation_settings::curve, curve_names},
			Number{"bias", &Saturation_settings::bias, Saturation_settings::default_bias, 0.0, 1.0},
			Number{"oversample", &Saturation_settings::oversample, Saturation_settings::default_oversample, 1, NAE_SAT_MAX_OS, power_of_two},
			Number{"output_db", &Saturation_settings::output_db, Saturation_settings::default_output_db, -24.0, 24.0},
			Number{"mix", &Saturation_settings::mix, Saturation_settings::default_mix, 0.0, 1.0},
		};
	}

	Json::Value Audio_saturation::serialize() const { return to_json(*this, saturation_fields); }
	void Audio_saturation::deserialize(const Json::Value& value) { Saturation_settings::operator=(from_json<Saturation_settings>(value, "Audio_saturation", saturation_fields)); }
	void Saturation_settings::clamp() { detail::clamp(*this, saturation_fields); }

	void Audio_saturation::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Saturation");
		// the latency is dropped in front; the flush's tail of as many frames completes the frames still owed
		run_on_handle<nae_sat>(
			io.input, io.output, stop_token, {"nae_sat", nae_sat_put, nae_sat_flush, nae_sat_available, nae_sat_receive, nae_sat_destroy}, "node",
			(size_t)nae_sat_latency(oversample),
			[&](nae_ctx* ctx, const Frame_data*, int ch)
			{
				nae_sat_params params;
				gpu::check(nae_sat_design(drive_db, bias, curve == Curve::Hard ? NAE_SAT_HARD : NAE_SAT_SOFT, oversample, output_db, mix, &params), "nae_sat_design");
				nae_sat* sat = nullptr;
				gpu::check(nae_sat_create(ctx, &params, ch, &sat), "nae_sat_create");
				return sat;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_gate
	infra::Processor::Info Audio_gate::get_processor_info()
	{
		return {"audio_gate", "Audio Gate", false, [] { return std::unique_ptr<infra::Processor>(new Audio_gate); },
				"Noise gate / downward expander: threshold, hysteresis, range, attack, hold, release, look-ahead (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_gate::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const gate_mode_names[] = {"gate", "expander"};
		constexpr std::tuple gate_fields{
			Choice{"mode", &Gate_settings::mode, gate_mode_names},
			Number{"threshold_db", &Gate_settings::threshold_db, Gate_settings::default_threshold_db, NAE_GATE_MIN_THRESHOLD_DB, NAE_GATE_MAX_THRESHOLD_DB},
			Number{"hysteresis_db", &Gate_settings::hysteresis_db, Gate_settings::default_hysteresis_db, 0.0, NAE_GATE_MAX_HYSTERESIS_DB},
			Number{"range_db", &Gate_settings::range_db, Gate_settings::default_range_db, 0.0, NAE_GATE_MAX_RANGE_DB},
			Number{"ratio", &Gate_settings::ratio, Gate_settings::default_ratio, 1.0, NAE_GATE_MAX_RATIO},
			Number{"attack_ms", &Gate_settings::attack_ms, Gate_settings::default_attack_ms, 0.0, 500.0},
			Number{"hold_ms", &Gate_settings::hold_ms, Gate_settings::default_hold_ms, 0.0, 10000.0},
			Number{"release_ms", &Gate_settings::release_ms, Gate_settings::default_release_ms, 1.0, 5000.0},
			Number{"lookahead_ms", &Gate_settings::lookahead_ms, Gate_settings::default_lookahead_ms, 0.0, 20.0},
			Flag{"link_channels", &Gate_settings::link_channels, true},
		};
	}

	Json::Value Audio_gate::serialize() const { return to_json(*this, gate_fields); }
	void Audio_gate::deserialize(const Json::Value& value) { Gate_settings::operator=(from_json<Gate_settings>(value, "Audio_gate", gate_fields)); }
	void Gate_settings::clamp() { detail::clamp(*this, gate_fields); }

	void Audio_gate::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Gate");
		run_on_handle<nae_gate>(
			io.input, io.output, stop_token, {"nae_gate", nae_gate_put, nae_gate_flush, nae_gate_available, nae_gate_receive, nae_gate_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				// the settings as the library's parameters at the stream's sample rate; a look-ahead too long for that rate is the user's error
				nae_gate_params params;
				const int rc = nae_gate_design(frame->sample_rate, mode == Mode::Expander ? NAE_GATE_MODE_EXPANDER : NAE_GATE_MODE_GATE, threshold_db,
											   hysteresis_db, range_db, ratio, attack_ms / 1000.0, hold_ms / 1000.0, release_ms / 1000.0, lookahead_ms / 1000.0,
											   link_channels ? 1 : 0, &params);
				if (rc == NAE_ERR_UNSUPPORTED)
					throw infra::Processor::Runtime_error("Look-ahead too long", "The look-ahead must not exceed 1024 samples at the stream's sample rate.",
										infra::fmt("lookahead %g ms, hold %g ms at %d Hz", lookahead_ms, hold_ms, frame->sample_rate));
				if (rc != NAE_OK)
					throw infra::Processor::Runtime_error("Invalid gate parameters", "A parameter of the gate node lies outside its range.",
										infra::fmt("nae_gate_design at %d Hz: code %d", frame->sample_rate, rc));
				nae_gate* gate = nullptr;
				gpu::check(nae_gate_create(ctx, &params, ch, &gate), "nae_gate_create");
				return gate;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_multiband
	infra::Processor::Info Audio_multiband::get_processor_info()
	{
		return {"audio_multiband", "Audio Multiband Compressor", false, [] { return std::unique_ptr<infra::Processor>(new Audio_multiband); },
				"Multiband compressor: two to four bands on Linkwitz-Riley crossovers, a compressor, a mute and a bypass per band (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_multiband::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		// A band's compressor keys are audio_dynamics' own fields, taken out of its one list: threshold_db, ratio, knee_db, attack_ms, release_ms
		// and makeup_db.  The mode, the look-ahead and the link are not a band's: the last two are the node's, for all bands.
		constexpr std::tuple multiband_band_dynamics_fields{std::get<1>(dynamics_fields), std::get<2>(dynamics_fields), std::get<3>(dynamics_fields),
															std::get<4>(dynamics_fields), std::get<5>(dynamics_fields), std::get<7>(dynamics_fields)};
		constexpr std::tuple multiband_band_flags{
			Flag{"mute", &Multiband_settings::Band::mute, false},
			Flag{"bypass", &Multiband_settings::Band::bypass, false},
		};
		constexpr std::tuple multiband_fields{
			Number{"lookahead_ms", &Multiband_settings::lookahead_ms, Multiband_settings::default_lookahead_ms, 0.0, 20.0},
			Flag{"link_channels", &Multiband_settings::link_channels, true},
		};

		Json::Value multiband_band_to_json(const Multiband_settings::Band& band)
		{
			Json::Value value = to_json(band.dynamics, multiband_band_dynamics_fields);
			std::apply([&](const auto&... f) { (f.write(band, value), ...); }, multiband_band_flags);
			return value;
		}

		// 1 ... 3 strictly ascending frequencies; absent: the default pair
		std::vector<double> multiband_crossovers_from_json(const Json::Value& value, const char* node_name)
		{
			if (!value.isMember("crossovers")) return Multiband_settings{}.crossovers;
			const Json::Value& list = value["crossovers"];
			if (!list.isArray() || list.size() < 1 || list.size() > Multiband_settings::max_crossovers) throw wrong_field(node_name, "crossovers");
			std::vector<double> crossovers;
			for (int i = 0; i < (int)list.size(); i++)
			{
				const Json::Value& f = list[i];
				if (!f.isDouble() || !(f.asDouble() >= Multiband_settings::min_crossover_hz && f.asDouble() <= Multiband_settings::max_crossover_hz) ||
					(!crossovers.empty() && !(f.asDouble() > crossovers.back())))
					throw wrong_field(node_name, "crossovers");
				crossovers.push_back(f.asDouble());
			}
			return crossovers;
		}

		// exactly n_bands objects; absent: every band at the defaults
		std::vector<Multiband_settings::Band> multiband_bands_from_json(const Json::Value& value, const char* node_name, size_t n_bands)
		{
			std::vector<Multiband_settings::Band> bands(n_bands);
			if (!value.isMember("bands")) return bands;
			const Json::Value& list = value["bands"];
			if (!list.isArray() || list.size() != n_bands) throw wrong_field(node_name, "bands");
			for (int b = 0; b < (int)list.size(); b++)
			{
				if (!list[b].isObject()) throw wrong_field(node_name, "bands");
				bands[b].dynamics = from_json<Dynamics_settings>(list[b], node_name, multiband_band_dynamics_fields);
				std::apply([&](const auto&... f) { (f.read(bands[b], list[b], node_name), ...); }, multiband_band_flags);
			}
			return bands;
		}
	}

	Json::Value Audio_multiband::serialize() const
	{
		Json::Value value = to_json<Multiband_settings>(*this, multiband_fields);
		if (crossovers != Multiband_settings{}.crossovers)
		{
			Json::Value list(Json::arrayValue);
			for (double f : crossovers) list.append(f);
			value["crossovers"] = list;
		}
		Json::Value list(Json::arrayValue);
		bool any = false;
		for (const Band& band : bands)
		{
			const Json::Value b = multiband_band_to_json(band);
			any = any || !b.isNull();
			list.append(b.isNull() ? Json::Value(Json::objectValue) : b);
		}
		if (any) value["bands"] = list;
		return value;
	}

	void Audio_multiband::deserialize(const Json::Value& value)
	{
		// everything is read and checked first: a rejected value leaves the node as it was
		Multiband_settings s = from_json<Multiband_settings>(value, "Audio_multiband", multiband_fields);
		s.crossovers = multiband_crossovers_from_json(value, "Audio_multiband");
		s.bands = multiband_bands_from_json(value, "Audio_multiband", s.crossovers.size() + 1);
		Multiband_settings::operator=(std::move(s));
	}

	void Multiband_settings::clamp()
	{
		detail::clamp(*this, multiband_fields);
		if (crossovers.empty()) crossovers = Multiband_settings{}.crossovers;
		if (crossovers.size() > max_crossovers) crossovers.resize(max_crossovers);
		for (double& f : crossovers) f = std::clamp(f, min_crossover_hz, max_crossover_hz);
		std::sort(crossovers.begin(), crossovers.end());
		bands.resize(crossovers.size() + 1);
		for (Band& band : bands) detail::clamp(band.dynamics, multiband_band_dynamics_fields);
	}

	void Audio_multiband::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Multiband Compressor");
		run_on_handle<nae_mb>(
			io.input, io.output, stop_token, {"nae_mb", nae_mb_put, nae_mb_flush, nae_mb_available, nae_mb_receive, nae_mb_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				// the settings as the library's parameters at the stream's sample rate: every band's compressor under the node's look-ahead and link
				// (design_dynamics: a look-ahead too long for that rate is the user's error), then the crossover tree
				nae_dyn_params band_params[NAE_MB_MAX_BANDS];
				unsigned mute_mask = 0, bypass_mask = 0;
				for (size_t b = 0; b < bands.size(); b++)
				{
					Dynamics_settings d = bands[b].dynamics;
					d.mode = Dynamics_settings::Mode::Compressor;
					d.lookahead_ms = lookahead_ms;
					d.link_channels = link_channels;
					band_params[b] = design_dynamics(d, frame->sample_rate);
					mute_mask |= (bands[b].mute ? 1u : 0u) << b;
					bypass_mask |= (bands[b].bypass ? 1u : 0u) << b;
				}
				nae_mb_params params;
				const int rc = nae_mb_design(frame->sample_rate, (int)bands.size(), crossovers.data(), band_params, mute_mask, bypass_mask, &params);
				if (rc != NAE_OK)
					throw infra::Processor::Runtime_error("Invalid crossover", "Every crossover must lie below half the stream's sample rate.",
										infra::fmt("nae_mb_design with %d bands, highest crossover %g Hz at %d Hz: code %d", (int)bands.size(), crossovers.back(),
												   frame->sample_rate, rc));
				nae_mb* mb = nullptr;
				gpu::check(nae_mb_create(ctx, &params, ch, &mb), "nae_mb_create");
				return mb;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_denoise
	infra::Processor::Info Audio_denoise::get_processor_info()
	{
		return {"audio_denoise", "Audio Noise Reduction", false, [] { return std::unique_ptr<infra::Processor>(new Audio_denoise); },
				"Noise reduction: a spectral gate against a noise profile learned from a stretch of the input, smoothed over time and frequency (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_denoise::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		// a frame size the library has; clamp falls back to the default
		constexpr bool is_stft_size(int n, int, int) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }
		constexpr Rule<int> stft_size{is_stft_size, [](int n, int lo, int hi) { return is_stft_size(n, lo, hi) ? n : Denoise_settings::default_fft_size; }};
		constexpr std::tuple denoise_fields{
			Number{"reduction_db", &Denoise_settings::reduction_db, Denoise_settings::default_reduction_db, 0.0, NAE_DENOISE_MAX_REDUCTION_DB},
			Number{"sensitivity_db", &Denoise_settings::sensitivity_db, Denoise_settings::default_sensitivity_db, NAE_DENOISE_MIN_SENSITIVITY_DB, NAE_DENOISE_MAX_SENSITIVITY_DB},
			Number{"fft_size", &Denoise_settings::fft_size, Denoise_settings::default_fft_size, 512, 4096, stft_size},
			Number{"time_smooth", &Denoise_settings::time_smooth, Denoise_settings::default_time_smooth, 0, NAE_DENOISE_MAX_TIME},
			Number{"freq_smooth", &Denoise_settings::freq_smooth, Denoise_settings::default_freq_smooth, 0, NAE_DENOISE_MAX_FREQ},
			Number{"profile_start_ms", &Denoise_settings::profile_start_ms, Denoise_settings::default_profile_start_ms, 0.0, 60000.0},
			Number{"profile_ms", &Denoise_settings::profile_ms, Denoise_settings::default_profile_ms, 20.0, 10000.0},
		};
	}

	Json::Value Audio_denoise::serialize() const { return to_json(*this, denoise_fields); }
	void Audio_denoise::deserialize(const Json::Value& value) { Denoise_settings::operator=(from_json<Denoise_settings>(value, "Audio_denoise", denoise_fields)); }
	void Denoise_settings::clamp() { detail::clamp(*this, denoise_fields); }

	void Audio_denoise::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Noise Reduction");
		gpu::Device_buffer d_profile;   // the learned profile: the handle copies it on the stream, so it stays until the node ends
		// the stretch the node learns from, in samples at the stream's rate
		const auto stretch = [&](const Frame_data* frame, size_t* start) {
			*start = (size_t)std::llround(profile_start_ms / 1000.0 * frame->sample_rate);
			return (size_t)std::llround(profile_ms / 1000.0 * frame->sample_rate);
		};
		run_on_handle_held<nae_denoise>(
			io.input, io.output, stop_token,
			{"nae_denoise", nae_denoise_put, nae_denoise_flush, nae_denoise_available, nae_denoise_receive, nae_denoise_destroy}, "node", 0,
			[&](const Frame_data* frame)
			{
				size_t start = 0;
				const size_t len = stretch(frame, &start);
				return start + len;
			},
			[&](nae_ctx* ctx, const Frame_data* frame, int ch, const float* samples, size_t total)
			{
				size_t start = 0;
				const size_t len = stretch(frame, &start);
				const size_t have = total > start ? std::min(len, total - start) : 0;
				if (have < (size_t)fft_size)
					throw Runtime_error("Noise profile too short", "The stream ended before the stretch the noise is learned from held one analysis frame.",
										infra::fmt("%d samples of the stretch at %g ms, fft_size %d", (int)have, profile_start_ms, fft_size));
				nae_denoise_params params;
				if (nae_denoise_design(reduction_db, sensitivity_db, fft_size, time_smooth, freq_smooth, &params) != NAE_OK)
					throw Runtime_error("Invalid noise reduction parameters", "A parameter of the noise reduction node lies outside its range.",
										infra::fmt("reduction %g dB, sensitivity %g dB, fft_size %d", reduction_db, sensitivity_db, fft_size));
				float* profile = static_cast<float*>(d_profile.reserve((size_t)ch * (fft_size / 2 + 1) * sizeof(float)));
				const nae_sig excerpt{const_cast<float*>(samples) + start * ch, 0, 1, (size_t)ch};
				gpu::check(nae_denoise_profile_f32(ctx, fft_size, &excerpt, have, ch, profile), "nae_denoise_profile_f32");
				nae_denoise* dn = nullptr;
				gpu::check(nae_denoise_create(ctx, &params, profile, ch, ch, &dn), "nae_denoise_create");
				return dn;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_separation
	infra::Processor::Info Audio_separation::get_processor_info()
	{
		return {"audio_separation", "Audio Separation", false, [] { return std::unique_ptr<infra::Processor>(new Audio_separation); },
				"Harmonic/percussive separation: a level for the tonal and one for the transient part, split by medians over time and frequency (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_separation::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		const char* const separation_mask_names[] = {"soft", "hard"};
		constexpr std::tuple separation_fields{
			Number{"harmonic_db", &Separation_settings::harmonic_db, Separation_settings::default_harmonic_db, NAE_HPSS_MIN_DB, NAE_HPSS_MAX_DB},
			Number{"percussive_db", &Separation_settings::percussive_db, Separation_settings::default_percussive_db, NAE_HPSS_MIN_DB, NAE_HPSS_MAX_DB},
			Choice{"mask", &Separation_settings::mask, separation_mask_names},
			Number{"fft_size", &Separation_settings::fft_size, Separation_settings::default_fft_size, 512, 4096, stft_size},   // the noise reduction's rule and default
			Number{"time_span", &Separation_settings::time_span, Separation_settings::default_time_span, 0, NAE_HPSS_MAX_SPAN},
			Number{"freq_span", &Separation_settings::freq_span, Separation_settings::default_freq_span, 0, NAE_HPSS_MAX_SPAN},
		};
		static_assert(Separation_settings::default_fft_size == Denoise_settings::default_fft_size, "stft_size clamps to the one default");
	}

	Json::Value Audio_separation::serialize() const { return to_json(*this, separation_fields); }
	void Audio_separation::deserialize(const Json::Value& value) { Separation_settings::operator=(from_json<Separation_settings>(value, "Audio_separation", separation_fields)); }
	void Separation_settings::clamp() { detail::clamp(*this, separation_fields); }

	void Audio_separation::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Separation");
		run_on_handle<nae_hpss>(
			io.input, io.output, stop_token, {"nae_hpss", nae_hpss_put, nae_hpss_flush, nae_hpss_available, nae_hpss_receive, nae_hpss_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data*, int ch)
			{
				nae_hpss_params params;
				if (nae_hpss_design(harmonic_db, percussive_db, fft_size, time_span, freq_span, mask == Mask::Hard ? 1 : 0, &params) != NAE_OK)
					throw infra::Processor::Runtime_error("Invalid separation parameters", "A parameter of the separation node lies outside its range.",
										infra::fmt("harmonic %g dB, percussive %g dB, fft_size %d", harmonic_db, percussive_db, fft_size));
				nae_hpss* hp = nullptr;
				gpu::check(nae_hpss_create(ctx, &params, ch, &hp), "nae_hpss_create");
				return hp;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_limiter
	infra::Processor::Info Audio_limiter::get_processor_info()
	{
		return {"audio_limiter", "Audio Limiter", false, [] { return std::unique_ptr<infra::Processor>(new Audio_limiter); },
				"True-peak look-ahead brickwall limiter: ceiling, drive, release, look-ahead, oversampled detector (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_limiter::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		constexpr std::tuple limiter_fields{
			Number{"ceiling_db", &Limiter_settings::ceiling_db, Limiter_settings::default_ceiling_db, NAE_LIM_MIN_CEILING_DB, NAE_LIM_MAX_CEILING_DB},
			Number{"gain_db", &Limiter_settings::gain_db, Limiter_settings::default_gain_db, -NAE_LIM_MAX_GAIN_DB, NAE_LIM_MAX_GAIN_DB},
			Number{"release_ms", &Limiter_settings::release_ms, Limiter_settings::default_release_ms, 1.0, 5000.0},
			Number{"lookahead_ms", &Limiter_settings::lookahead_ms, Limiter_settings::default_lookahead_ms, 0.0, 20.0},
			Flag{"true_peak", &Limiter_settings::true_peak, true},
			Flag{"link_channels", &Limiter_settings::link_channels, true},
		};
	}

	Json::Value Audio_limiter::serialize() const { return to_json(*this, limiter_fields); }
	void Audio_limiter::deserialize(const Json::Value& value) { Limiter_settings::operator=(from_json<Limiter_settings>(value, "Audio_limiter", limiter_fields)); }
	void Limiter_settings::clamp() { detail::clamp(*this, limiter_fields); }

	void Audio_limiter::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Limiter");
		run_on_handle<nae_lim>(
			io.input, io.output, stop_token, {"nae_lim", nae_lim_put, nae_lim_flush, nae_lim_available, nae_lim_receive, nae_lim_destroy}, "node", 0,
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				// the settings as the library's parameters at the stream's sample rate; a look-ahead too long for that rate is the user's error
				nae_lim_params params;
				const int rc = nae_lim_design(frame->sample_rate, ceiling_db, gain_db, release_ms / 1000.0, lookahead_ms / 1000.0, true_peak ? 1 : 0,
											  link_channels ? 1 : 0, &params);
				if (rc == NAE_ERR_UNSUPPORTED)
					throw infra::Processor::Runtime_error("Look-ahead too long", "The look-ahead must not exceed 1018 samples at the stream's sample rate.",
										infra::fmt("lookahead %g ms at %d Hz", lookahead_ms, frame->sample_rate));
				if (rc != NAE_OK)
					throw infra::Processor::Runtime_error("Invalid limiter parameters", "A parameter of the limiter node lies outside its range.",
										infra::fmt("nae_lim_design at %d Hz: code %d", frame->sample_rate, rc));
				nae_lim* lim = nullptr;
				gpu::check(nae_lim_create(ctx, &params, ch, &lim), "nae_lim_create");
				return lim;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_dither
	infra::Processor::Info Audio_dither::get_processor_info()
	{
		return {"audio_dither", "Audio Dither", false, [] { return std::unique_ptr<infra::Processor>(new Audio_dither); },
				"Word-length reduction: TPDF dither and noise-shaped requantisation to 8 ... 24 bits (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_dither::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		// the library's kind of each name, in the enumerators' order (the default first)
		const char* const dither_kind_names[] = {"triangular", "none", "rectangular", "highpass"};
		constexpr int dither_kinds[] = {NAE_DITHER_TRIANGULAR, NAE_DITHER_NONE, NAE_DITHER_RECTANGULAR, NAE_DITHER_HIGHPASS};
		const char* const dither_shaping_names[] = {"none", "first", "second", "lipshitz"};

		// 1 ... NAE_DITHER_MAX_TAPS finite numbers whose absolute sum is at most NAE_DITHER_MAX_TAP_SUM; no key is no taps, and no taps are not written;
		// not clamped
		struct Dither_taps
		{
			const char* key;

			void write(const Dither_settings& r, Json::Value& value) const
			{
				if (r.taps.empty()) return;
				Json::Value a(Json::arrayValue);
				for (double c : r.taps) a.append(c);
				value[key] = a;
			}
			void read(Dither_settings& r, const Json::Value& value, const char* node_name) const
			{
				r.taps.clear();
				if (!value.isMember(key)) return;
				const Json::Value& a = value[key];
				if (!a.isArray() || a.size() < 1 || a.size() > NAE_DITHER_MAX_TAPS) throw wrong_field(node_name, key);
				double sum = 0;
				const int n = (int)a.size();
				for (int k = 0; k < n; k++)
				{
					if (!a[k].isDouble() || !std::isfinite(a[k].asDouble())) throw wrong_field(node_name, key);
					sum += std::fabs(a[k].asDouble());
				}
				if (!(sum <= NAE_DITHER_MAX_TAP_SUM)) throw wrong_field(node_name, key);
				for (int k = 0; k < n; k++) r.taps.push_back(a[k].asDouble());
			}
			void keep(Dither_settings&) const {}
		};
		// an exact integer below 2^53, written as a double; not clamped
		struct Dither_seed
		{
			const char* key;

			void write(const Dither_settings& r, Json::Value& value) const { if (r.seed != Dither_settings::default_seed) value[key] = (double)r.seed; }
			void read(Dither_settings& r, const Json::Value& value, const char* node_name) const
			{
				r.seed = Dither_settings::default_seed;
				if (!value.isMember(key)) return;
				// compared as a double with the range first: a number outside the integer range is never converted
				const Json::Value& v = value[key];
				if (!v.isDouble() || !(v.asDouble() >= 0.0 && v.asDouble() < 9007199254740992.0) || v.asDouble() != (double)(uint64_t)v.asDouble()) throw wrong_field(node_name, key);
				r.seed = (uint64_t)v.asDouble();
			}
			void keep(Dither_settings&) const {}
		};
		constexpr std::tuple dither_fields{
			Number{"bits", &Dither_settings::bits, Dither_settings::default_bits, NAE_DITHER_MIN_BITS, NAE_DITHER_MAX_BITS},
			Choice{"dither", &Dither_settings::dither, dither_kind_names},
			Choice{"shaping", &Dither_settings::shaping, dither_shaping_names},
			Dither_taps{"taps"},
			Dither_seed{"seed"},
		};
	}

	Json::Value Audio_dither::serialize() const { return to_json(*this, dither_fields); }
	void Audio_dither::deserialize(const Json::Value& value) { Dither_settings::operator=(from_json<Dither_settings>(value, "Audio_dither", dither_fields)); }
	void Dither_settings::clamp() { detail::clamp(*this, dither_fields); }

	void Audio_dither::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "Audio Dither");
		run_on_handle<nae_dither>(
			io.input, io.output, stop_token, {"nae_dither", nae_dither_put, nae_dither_flush, nae_dither_available, nae_dither_receive, nae_dither_destroy},
			"node", 0,
			[&](nae_ctx* ctx, const Frame_data*, int ch)
			{
				// the preset's record, then the taps of the node's own where it has them: no sample rate enters
				nae_dither_params params;
				const int rc = nae_dither_design(bits, dither_kinds[(size_t)dither], (int)shaping, seed, &params);
				if (rc != NAE_OK)
					throw infra::Processor::Runtime_error("Invalid dither parameters", "A parameter of the dither node lies outside its range.",
										infra::fmt("nae_dither_design: code %d", rc));
				if (!taps.empty())
				{
					params.n_taps = (int)taps.size();
					for (size_t k = 0; k < taps.size(); k++) params.taps[k] = taps[k];
				}
				nae_dither* d = nullptr;
				gpu::check(nae_dither_create(ctx, &params, ch, &d), "nae_dither_create");
				return d;
			}
		);
	}

	// ------------------------------------------------------------------------------------------ Audio_loudness
	infra::Processor::Info Audio_loudness::get_processor_info()
	{
		return {"audio_loudness", "Audio Loudness", false, [] { return std::unique_ptr<infra::Processor>(new Audio_loudness); },
				"Loudness normalization: ITU-R BS.1770 integrated loudness and true peak, one gain to a target level under a true-peak ceiling (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_loudness::get_pin_attributes() const { return io_pins(); }

	namespace
	{
		constexpr std::tuple loudness_fields{
			Number{"target_lufs", &Loudness_settings::target_lufs, Loudness_settings::default_target_lufs, NAE_LOUD_MIN_TARGET_LUFS, NAE_LOUD_MAX_TARGET_LUFS},
			Number{"true_peak_db", &Loudness_settings::true_peak_db, Loudness_settings::default_true_peak_db, NAE_LOUD_MIN_CEILING_DBTP, 0.0},
			Number{"max_gain_db", &Loudness_settings::max_gain_db, Loudness_settings::default_max_gain_db, 0.0, NAE_LOUD_MAX_GAIN_DB},
		};
	}

	Json::Value Audio_loudness::serialize() const { return to_json(*this, loudness_fields); }
	void Audio_loudness::deserialize(const Json::Value& value) { Loudness_settings::operator=(from_json<Loudness_settings>(value, "Audio_loudness", loudness_fields)); }
	void Loudness_settings::clamp() { detail::clamp(*this, loudness_fields); }

	void Audio_loudness::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		// this node's context (own stream) is made when the first gating block has arrived: a shorter stream never touches the GPU.  First
		// local, destroyed last — after the handle guard and the buffers
		std::optional<gpu::Node> node;
		const Node_streams io = node_streams(input, output, "Audio Loudness");
		nae_loud* h = nullptr;
		struct Guard { nae_loud*& h; ~Guard() { if (h) nae_loud_destroy(h); } } guard{h};
		struct Buffers { gpu::Device_buffer d_raw, d_f32; gpu::Pinned_buffer h_raw, h_f32; };
		std::optional<Buffers> buf;
		Intake in;                  // its shapes are every frame received: nothing leaves before the end
		std::vector<float> kept;    // their samples as interleaved f32, from the first put on
		// the frames wait for one gating block: NAE_LOUD_BLOCK_SUBS sub-blocks of 1 / NAE_LOUD_SUBS_PER_S seconds, rounded up to whole samples
		const auto gating_block = [](const Frame_data* frame) {
			const size_t per_s = (size_t)NAE_LOUD_BLOCK_SUBS * frame->sample_rate;
			return per_s / NAE_LOUD_SUBS_PER_S + (per_s % NAE_LOUD_SUBS_PER_S != 0);
		};

		while (!stop_token)
		{
			if (!take_in(in, io.input, "node", gating_block)) continue;
			// one gain from one meter: the K-weighting and the sub-block are the first frame's rate's
			for (const auto& f : in.pending)
				if (f->data()->sample_rate != in.shapes.front().sample_rate)
					throw Runtime_error("Sample rate changed", "The node runs one stream of a fixed sample rate.",
										infra::fmt("Got %d Hz after %d Hz", f->data()->sample_rate, in.shapes.front().sample_rate));
			if (!in.pending.empty() && (h != nullptr || in.pending_samples >= in.need))
			{
				if (h == nullptr)
				{
					const int sample_rate = in.shapes.front().sample_rate;
					nae_loud_params params;
					const int rc = nae_loud_design(sample_rate, target_lufs, true_peak_db, max_gain_db, &params);
					if (rc == NAE_ERR_UNSUPPORTED)
						throw Runtime_error("Unsupported sample rate", "The loudness meter runs at 8000 ... 192000 Hz, in multiples of 10 Hz.",
											infra::fmt("%d Hz", sample_rate));
					if (rc != NAE_OK)
						throw Runtime_error("Invalid loudness parameters", "A parameter of the loudness node lies outside its range.",
											infra::fmt("nae_loud_design at %d Hz: code %d", sample_rate, rc));
					node.emplace();
					buf.emplace();
					gpu::check(nae_loud_create(node->ctx(), &params, in.ch, &h), "nae_loud_create");
				}
				size_t total = 0;
				float* samples = upload_as_f32(in.pending, buf->h_raw, buf->d_raw, buf->d_f32, &total);
				gpu::check(nae_loud_put(h, samples, total), "nae_loud_put");
				// the node keeps the f32 samples the meter saw.  Packed float frames (and mono planar ones) already are those samples; integer
				// and planar stereo frames were converted on the device and come back from there.  Either way the batch is waited for: the
				// staging buffers are reused by the next one
				bool wire = true;
				for (const auto& f : in.pending)
					wire = wire && (f->data()->format == AV_SAMPLE_FMT_FLT || (f->data()->format == AV_SAMPLE_FMT_FLTP && in.ch == 1));
				if (wire)
				{
					gpu::wait(stop_token);
					for (const auto& f : in.pending)
					{
						const float* data = reinterpret_cast<const float*>(f->data()->data[0]);
						kept.insert(kept.end(), data, data + (size_t)f->data()->nb_samples * in.ch);
					}
				}
				else
				{
					float* host = static_cast<float*>(buf->h_f32.reserve(total * in.ch * sizeof(float)));
					gpu::check(nae_memcpy_d2h(node->ctx(), host, samples, total * in.ch * sizeof(float)), "d2h");
					gpu::wait(stop_token);
					kept.insert(kept.end(), host, host + total * in.ch);
				}
				in.pending.clear();
				in.pending_samples = 0;
			}
			if (in.at_end)
			{
				if (h == nullptr)
				{
					// under 400 ms: no gating block, no loudness — the frames pass as they are
					for (const auto& f : in.pending) push_to_all(io.output, f, stop_token);
					break;
				}
				gpu::check(nae_loud_flush(h), "nae_loud_flush");
				gpu::wait(stop_token);
				nae_loud_result result;
				gpu::check(nae_loud_get_result(h, &result), "nae_loud_get_result");
				for (float& v : kept) v *= result.gain_f32;   // one f32 product, as loud_apply_kernel's
				cut_and_push(in.shapes, kept.data(), kept.size() / in.ch, in.ch, io.output, stop_token);
				break;
			}
		}
		for (auto& stream : io.output) stream->set_eof();
	}
}
