#include "audio-velocity.hpp"
#include "node-util.hpp"
#include "velocity-cadence.hpp"

#include <algorithm>
#include <cmath>

namespace processor
{
	using namespace detail;

	const char* algorithm_name(Stretch_algorithm a) { return a == Stretch_algorithm::Soundtouch ? "soundtouch" : "vocoder"; }

	namespace
	{
		Stretch_algorithm g_default_algorithm = Stretch_algorithm::Vocoder;
	}
	Stretch_algorithm default_stretch_algorithm() { return g_default_algorithm; }
	void set_default_stretch_algorithm(Stretch_algorithm a) { g_default_algorithm = a; }

	Stretch_algorithm algorithm_from_json(const Json::Value& value)
	{
		if (value.isMember("algorithm") && value["algorithm"].isString())
		{
			if (value["algorithm"].asString() == "soundtouch") return Stretch_algorithm::Soundtouch;
			if (value["algorithm"].asString() == "vocoder") return Stretch_algorithm::Vocoder;
		}
		return default_stretch_algorithm();   // no key: a project saved by the reference
	}

	bool phase_lock_from_json(const Json::Value& value, const char* node_name) { return bool_from_json(value, node_name, "phase_lock"); }
	bool formant_from_json(const Json::Value& value, const char* node_name) { return bool_from_json(value, node_name, "formant"); }
	bool transients_from_json(const Json::Value& value, const char* node_name) { return bool_from_json(value, node_name, "transients"); }
	bool link_channels_from_json(const Json::Value& value, const char* node_name) { return bool_from_json(value, node_name, "link_channels"); }

	float formant_shift_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("formant_shift")) return 0;
		if (!value["formant_shift"].isDouble()) throw wrong_field(node_name, "formant_shift");
		const float semitones = value["formant_shift"].asFloat();
		if (!(semitones >= -24.0f && semitones <= 24.0f))
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " accepts a formant shift between -24 and 24 semitones.",
				"Out of range: formant_shift"
			);
		return semitones;
	}

	int fft_size_from_json(const Json::Value& value, const char* node_name, bool phase_lock)
	{
		if (!value.isMember("fft_size")) return 1024;
		const Json::Value& v = value["fft_size"];
		// compared as a double with the sizes first: a number outside int's range is never converted
		int n = 0;
		if (v.isDouble())
			for (int size : {512, 1024, 2048, 4096})
				if (v.asDouble() == (double)size) n = size;
		if (n == 0 || (phase_lock && n != 1024)) throw wrong_field(node_name, "fft_size");
		return n;
	}

	namespace
	{
		// construct_audio_frame_float, audio-velocity.cpp:234-263 (time_us is a FLOAT there: 24-bit pts quirk kept)
		std::shared_ptr<Audio_frame> construct_audio_frame_float(const float* samples, size_t n_frames, int sample_rate,
																 int channel_count, float time_us)
		{
			return make_f32_frame(samples, static_cast<int>(n_frames), channel_count, sample_rate, static_cast<int64_t>(time_us), {1, 1000000});
		}

		// the object soundtouch_process_payload talks to: the phase-vocoder handle (default) or the
		// SoundTouch-shaped WSOLA chain, chosen by the node's "algorithm" key
		struct Stretcher
		{
			nae_stretch* pv = nullptr;
			nae_wsola* st = nullptr;
			~Stretcher()
			{
				if (pv) nae_stretch_destroy(pv);
				if (st) nae_wsola_destroy(st);
			}
			bool open() const { return pv != nullptr || st != nullptr; }
			void create(Stretch_algorithm algo, bool phase_lock, int fft_size, bool formant, bool transients, bool link_channels, float formant_shift,
						int sample_rate, int channels, float velocity, float pitch)
			{
				const unsigned flags = (phase_lock ? NAE_STRETCH_PHASE_LOCK : 0u) | (transients ? NAE_STRETCH_TRANSIENTS : 0u)
									   | (link_channels ? NAE_STRETCH_LINK_CHANNELS : 0u);
				// (phase_lock, fft_size, formant, formant_shift, transients and link_channels are vocoder options: the WSOLA chain has none)
				if (algo == Stretch_algorithm::Soundtouch)
					gpu::check(nae_wsola_create(gpu::context(), sample_rate, channels, velocity, pitch, &st), "nae_wsola_create");
				else if (formant_shift != 0)   // the envelope stage with the default lifter, whether or not "formant" is set
					gpu::check(nae_stretch_create_formant_shift(gpu::context(), sample_rate, channels, velocity, pitch, flags, fft_size,
																nae_stretch_formant_lifter(sample_rate, fft_size),
																std::pow(2.0, (double)formant_shift / 12.0), &pv),
							   "nae_stretch_create_formant_shift");
				else if (formant)
					gpu::check(nae_stretch_create_formant(gpu::context(), sample_rate, channels, velocity, pitch, flags, fft_size,
														  nae_stretch_formant_lifter(sample_rate, fft_size), &pv),
							   "nae_stretch_create_formant");
				else
					gpu::check(nae_stretch_create_n(gpu::context(), sample_rate, channels, velocity, pitch, flags, fft_size, &pv),
							   "nae_stretch_create_n");
			}
			size_t available() const { return pv ? nae_stretch_available(pv) : nae_wsola_available(st); }
			void put(const float* samples, size_t n)
			{
				gpu::check(pv ? nae_stretch_put(pv, samples, n) : nae_wsola_put(st, samples, n), "stretch put");
			}
			void receive_device(float* dst, size_t max, size_t* got)
			{
				gpu::check(pv ? nae_stretch_receive(pv, dst, max, got) : nae_wsola_receive(st, dst, max, got), "stretch receive");
			}
			void flush() { gpu::check(pv ? nae_stretch_flush(pv) : nae_wsola_flush(st), "stretch flush"); }
		};

		// soundtouch_process_payload, audio-velocity.cpp:265-443, with a GPU handle in SoundTouch's place
		void stretch_process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token, float velocity, float pitch, const std::string& processor_name,
			Stretch_algorithm algorithm, bool phase_lock, int fft_size, bool formant, bool transients, bool link_channels, float formant_shift,
			Batch_stats& batch_stats
		)
		{
			gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
			batch_stats = {};
			const Node_streams io = node_streams(input, output, processor_name);
			Stretcher soundtouch;
			gpu::Device_buffer d_raw, d_f32, d_out;
			gpu::Pinned_buffer h_raw, h_out;
			bool input_stream_eof = false, pending_put = false;
			Frame_ptr held;  // popped, but with another channel count than the batch in front of it
			int channel_count = 0, sample_rate = 0;
			double time_seconds = 0.0;

			// receiveSamples + construct_audio_frame_float + push (:294-316), for every chunk that is ready at once: the chunk sizes are
			// those the reference's loop would take one per turn (min(numSamples, max) while more than `floor` samples are queued); all
			// of them come down as ONE asynchronous copy into page-locked staging behind ONE wait, then they are cut into frames
			const cadence::Bounds chunk_bounds = cadence::bounds(velocity);  // :416-417
			auto acquire_chunks = [&](size_t floor)
			{
				const std::vector<size_t> chunks = cadence::drain(soundtouch.available(), floor, chunk_bounds);
				size_t total = 0;
				for (const size_t take : chunks) total += take;
				if (chunks.empty()) return;
				nae_ctx* ctx = gpu::context();
				float* dev = static_cast<float*>(d_out.reserve(total * channel_count * sizeof(float)));
				float* host = static_cast<float*>(h_out.reserve(total * channel_count * sizeof(float)));
				size_t got = 0;
				soundtouch.receive_device(dev, total, &got);
				gpu::check(nae_memcpy_d2h(ctx, host, dev, got * channel_count * sizeof(float)), "d2h");
				gpu::wait(stop_token);
				size_t pos = 0;
				for (const size_t take : chunks)
				{
					const size_t n = std::min(take, got - pos);
					if (n == 0) break;
					auto new_frame = construct_audio_frame_float(host + pos * channel_count, n, sample_rate, channel_count, (float)(time_seconds * 1000000));
					time_seconds += double(n) / sample_rate;
					pos += n;
					push_to_all(io.output, new_frame, stop_token);
				}
			};

			while (!stop_token)
			{
				if (!input_stream_eof || held)
				{
					// Batching: the reference puts one frame per round; here every frame that is already waiting
					// (at most 16) is uploaded, converted and put as ONE block behind one wait.  The handle's output does not
					// depend on how its input is cut into puts (tests/test_gpu_stft.py, test_gpu_wsola.py: chunking invariance).
					const std::vector<Frame_ptr> batch = collect_batch(io.input, held, &input_stream_eof);
					if (!batch.empty())
					{
						constexpr size_t max_queued_samples = 65536;
						const Frame_data* frame = batch.front()->data();
						if (!soundtouch.open())
						{
							if (frame->sample_rate < 8000 || frame->sample_rate > 48000)  // :371-379
								throw infra::Processor::Runtime_error(
									"Unsupported sample rate",
									infra::fmt("%d requires a sample rate between 8000 and 48000 Hz.", frame->sample_rate),
									infra::fmt("Sample rate: %d", frame->sample_rate)
								);
							soundtouch.create(algorithm, phase_lock, fft_size, formant, transients, link_channels, formant_shift, frame->sample_rate, frame->ch_layout.nb_channels, velocity, pitch);
							channel_count = frame->ch_layout.nb_channels;
							time_seconds = frame->pts * av_q2d(frame->time_base);
							sample_rate = frame->sample_rate;
						}
						// (:399-400 waits while more than 65536 samples are queued in SoundTouch.  Only this fiber takes samples out, and a
						// batched put adds up to 16 frames at once, so instead of waiting the loop below receives until the queue is
						// under one chunk again: the queue never grows beyond one batch.)
						static_assert(max_queued_samples >= 16 * 1152 * 3, "a batch fits the reference's queue bound");
						size_t total = 0;
						float* samples = upload_as_f32(batch, h_raw, d_raw, d_f32, &total);
						soundtouch.put(samples, total);
						// (no wait here: the frames were copied into page-locked staging and are released; staging and device buffers are
						// next touched behind the wait of the receive below, or of the next turn's)
						pending_put = true;
						batch_stats.rounds += batch.size();
					}
				}
				if (soundtouch.open())
				{
					// (:414 "numSamples() == 0 && eof -> break" is subsumed by the flush branch)
					const uint32_t min_samples = chunk_bounds.min_samples;
					if (soundtouch.available() > min_samples)
					{
						// the reference receives one chunk per loop turn because it puts one frame per turn (:403,416-424); a batched put
						// makes several chunks available, and all of them are taken now (chunk sizes stay inside [min, max])
						acquire_chunks(min_samples);
						pending_put = false;
						batch_stats.waits++;
					}
					else if (input_stream_eof)
					{
						soundtouch.flush();
						// the reference emits ONE frame with everything that is left (:427-433); here flush() may release
						// the whole stream, so it is cut into the same [min, max] chunks the steady state uses
						acquire_chunks(0);
						break;
					}
					if (pending_put)
					{
						// a put that released nothing: its staging is reused by the next batch, so it is waited for now
						gpu::wait(stop_token);
						pending_put = false;
						batch_stats.waits++;
					}
				}
				else if (input_stream_eof)
					break;
				nae_fiber::this_fiber::yield();
			}
			for (auto& stream : io.output) stream->set_eof();
		}
	}

	// ------------------------------------------------------------------------------------------ Velocity_modifier
	infra::Processor::Info Velocity_modifier::get_processor_info()
	{
		return {"velocity_modifier", "Velocity Modifier", false,
				[] { return std::unique_ptr<infra::Processor>(new Velocity_modifier); }, "Audio Velocity Modifier (MI355X)"};
	}
	std::vector<infra::Processor::Pin_attribute> Velocity_modifier::get_pin_attributes() const { return io_pins(); }

	void Velocity_modifier::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		stretch_process_payload(input, output, stop_token, velocity, keep_pitch ? 1 / velocity : 1, get_processor_info().display_name,
								algorithm, phase_lock, fft_size, false, transients, link_channels, 0, batch_stats);  // :452-459
	}

	Json::Value Velocity_modifier::serialize() const
	{
		Json::Value value;
		value["velocity"] = velocity;
		value["keep_pitch"] = keep_pitch;
		if (algorithm != default_stretch_algorithm()) value["algorithm"] = algorithm_name(algorithm);
		if (phase_lock) value["phase_lock"] = true;
		if (fft_size != 1024) value["fft_size"] = fft_size;
		if (transients) value["transients"] = true;
		if (link_channels) value["link_channels"] = true;
		return value;
	}

	void Velocity_modifier::deserialize(const Json::Value& value)
	{
		if (value.isMember("velocity") && value["velocity"].isDouble()) velocity = value["velocity"].asFloat();
		if (value.isMember("keep_pitch") && value["keep_pitch"].isBool()) keep_pitch = value["keep_pitch"].asBool();
		algorithm = algorithm_from_json(value);
		phase_lock = phase_lock_from_json(value, "Velocity_modifier");
		fft_size = fft_size_from_json(value, "Velocity_modifier", phase_lock);
		transients = transients_from_json(value, "Velocity_modifier");
		link_channels = link_channels_from_json(value, "Velocity_modifier");
	}

	// ------------------------------------------------------------------------------------------ Pitch_modifier
	infra::Processor::Info Pitch_modifier::get_processor_info()
	{
		return {"pitch_modifier", "Pitch Modifier", false, [] { return std::unique_ptr<infra::Processor>(new Pitch_modifier); },
				"Audio Pitch Modifier (MI355X)"};
	}
	std::vector<infra::Processor::Pin_attribute> Pitch_modifier::get_pin_attributes() const { return io_pins(); }

	void Pitch_modifier::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		stretch_process_payload(input, output, stop_token, 1, std::pow(2.0f, pitch / 12.0f), get_processor_info().display_name,
								algorithm, phase_lock, fft_size, formant, transients, link_channels, formant_shift, batch_stats);  // :469-476
	}

	Json::Value Pitch_modifier::serialize() const
	{
		Json::Value value;
		value["pitch"] = pitch;
		if (algorithm != default_stretch_algorithm()) value["algorithm"] = algorithm_name(algorithm);
		if (phase_lock) value["phase_lock"] = true;
		if (fft_size != 1024) value["fft_size"] = fft_size;
		if (formant) value["formant"] = true;
		if (formant_shift != 0) value["formant_shift"] = formant_shift;
		if (transients) value["transients"] = true;
		if (link_channels) value["link_channels"] = true;
		return value;
	}
	void Pitch_modifier::deserialize(const Json::Value& value)
	{
		if (value.isMember("pitch") && value["pitch"].isDouble()) pitch = value["pitch"].asFloat();
		algorithm = algorithm_from_json(value);
		phase_lock = phase_lock_from_json(value, "Pitch_modifier");
		fft_size = fft_size_from_json(value, "Pitch_modifier", phase_lock);
		formant = formant_from_json(value, "Pitch_modifier");
		formant_shift = formant_shift_from_json(value, "Pitch_modifier");
		transients = transients_from_json(value, "Pitch_modifier");
		link_channels = link_channels_from_json(value, "Pitch_modifier");
	}

	// ------------------------------------------------------------------------------------------ Audio_spectrum
	infra::Processor::Info Audio_spectrum::get_processor_info()
	{
		return {"audio_spectrum", "FFT Spectrum", false, [] { return std::unique_ptr<infra::Processor>(new Audio_spectrum); },
				"Hann-windowed magnitude spectrum, 256 to 4096 points, any hop (MI355X)"};
	}
	std::vector<infra::Processor::Pin_attribute> Audio_spectrum::get_pin_attributes() const { return io_pins(); }

	Json::Value Audio_spectrum::serialize() const
	{
		Json::Value value;
		if (fft_size != default_fft_size) value["fft_size"] = fft_size;
		if (hop != default_hop) value["hop"] = hop;
		return value;
	}

	void Audio_spectrum::deserialize(const Json::Value& value)
	{
		const auto wrong = [](const char* field) { return wrong_field("Audio_spectrum", field); };
		// no key: the default (a project saved before the key existed).  The ranges are the widest nae_spectrum_frames_ex accepts anything in
		const int n = int_from_json(value, "Audio_spectrum", "fft_size", 256, 4096, default_fft_size);
		const int h = int_from_json(value, "Audio_spectrum", "hop", 1, 4096, default_hop);
		if (nae_spectrum_frames_ex((size_t)n, n, 1) == 0) throw wrong("fft_size");
		if (nae_spectrum_frames_ex((size_t)n, n, h) == 0) throw wrong("hop");
		fft_size = n;
		hop = h;
	}

	void Audio_spectrum::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // first local, destroyed last (gpu-context.hpp)
		const Node_streams io = node_streams(input, output, "FFT Spectrum");
		nae_ctx* ctx = gpu::context();
		last_context = ctx;
		nae_spectrum* spectrum = nullptr;
		struct Guard { nae_spectrum*& h; ~Guard() { if (h) nae_spectrum_destroy(h); } } guard{spectrum};
		gpu::Device_buffer d_raw, d_f32, d_out;
		gpu::Pinned_buffer h_raw, h_out;
		int ch = 0, sample_rate = 0;
		double time_seconds = 0.0;
		Frame_ptr held;  // popped, but with another channel count than the batch in front of it

		while (!stop_token)
		{
			bool ended = false;
			const std::vector<Frame_ptr> batch = collect_batch(io.input, held, &ended);
			if (batch.empty())
			{
				if (ended) break;  // a trailing partial window produces no frame
				nae_fiber::this_fiber::yield();
				continue;
			}
			const Frame_data* frame = batch.front()->data();
			if (spectrum == nullptr)
			{
				ch = frame->ch_layout.nb_channels;
				if (ch != 1 && ch != 2) throw Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels", ch));
				sample_rate = frame->sample_rate;
				time_seconds = frame->pts * av_q2d(frame->time_base);
				gpu::check(nae_spectrum_create(ctx, fft_size, hop, ch, &spectrum), "nae_spectrum_create");
			}
			size_t total = 0;
			float* samples = upload_as_f32(batch, h_raw, d_raw, d_f32, &total);
			gpu::check(nae_spectrum_put(spectrum, samples, total), "nae_spectrum_put");
			const size_t ready = nae_spectrum_available(spectrum);
			if (ready == 0) { gpu::wait(stop_token); continue; }
			const int bins = fft_size / 2 + 1;
			const size_t rec = (size_t)ch * bins;
			float* dout = static_cast<float*>(d_out.reserve(ready * rec * sizeof(float)));
			float* host = static_cast<float*>(h_out.reserve(ready * rec * sizeof(float)));
			size_t got = 0;
			gpu::check(nae_spectrum_receive(spectrum, dout, ready, &got), "nae_spectrum_receive");
			gpu::check(nae_memcpy_d2h(ctx, host, dout, got * rec * sizeof(float)), "d2h");
			gpu::wait(stop_token);
			for (size_t f = 0; f < got && !stop_token; f++)
			{
				push_to_all(io.output, make_f32_frame(host + f * rec, bins, ch, sample_rate, (int64_t)(time_seconds * 1000000), {1, 1000000}, true), stop_token);
				time_seconds += (double)hop / sample_rate;
			}
		}
		for (auto& stream : io.output) stream->set_eof();
	}
}
