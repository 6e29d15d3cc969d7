#include "audio-velocity.hpp"
#include <type_traits>
#include "audio-filter.hpp"
#include "audio-reverb.hpp"
#include "audio-eq.hpp"
#include "audio-dynamics.hpp"
#include "gpu-context.hpp"
#include "velocity-cadence.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>

namespace processor
{
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

	bool phase_lock_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("phase_lock")) return false;
		if (!value["phase_lock"].isBool())
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: phase_lock"
			);
		return value["phase_lock"].asBool();
	}

	bool formant_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("formant")) return false;
		if (!value["formant"].isBool())
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: formant"
			);
		return value["formant"].asBool();
	}

	bool transients_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("transients")) return false;
		if (!value["transients"].isBool())
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: transients"
			);
		return value["transients"].asBool();
	}

	bool link_channels_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("link_channels")) return false;
		if (!value["link_channels"].isBool())
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: link_channels"
			);
		return value["link_channels"].asBool();
	}

	float formant_shift_from_json(const Json::Value& value, const char* node_name)
	{
		if (!value.isMember("formant_shift")) return 0;
		if (!value["formant_shift"].isDouble())
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: formant_shift"
			);
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
		if (n == 0 || (phase_lock && n != 1024))
			throw infra::Processor::Runtime_error(
				"Failed to deserialize JSON file",
				std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
				"Wrong field: fft_size"
			);
		return n;
	}

	namespace
	{
		std::vector<infra::Processor::Pin_attribute> io_pins()
		{
			return {
				{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
				{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
			};
		}

		// construct_audio_frame_float, audio-velocity.cpp:234-263 (time_us is a FLOAT there: 24-bit pts quirk kept)
		std::shared_ptr<Audio_frame> construct_audio_frame_float(const float* samples, size_t n_frames, int sample_rate,
																 int channel_count, float time_us)
		{
			auto new_frame = std::make_shared<Audio_frame>();
			Frame_data* frame = new_frame->data();
			frame->sample_rate = sample_rate;
			frame->ch_layout.nb_channels = channel_count;
			frame->nb_samples = static_cast<int>(n_frames);
			frame->format = AV_SAMPLE_FMT_FLT;
			frame->time_base = {1, 1000000};
			frame->pts = static_cast<int64_t>(time_us);
			frame_get_buffer(frame, 32);
			std::memcpy(frame->data[0], samples, n_frames * channel_count * sizeof(float));
			return new_frame;
		}

		// frames -> device interleaved f32, one after the other (extract_samples_interleaved, :150-232).  The frames of a batch are
		// copied into page-locked staging on the CPU and go up as ONE asynchronous copy; on the device
		//   * packed float frames (and mono planar ones) already ARE the interleaved signal: no kernel at all;
		//   * a run of planar stereo float frames of equal length is interleaved by ONE strided launch (frames as "streams");
		//   * integer formats: nae_to_f32_interleaved per frame (the reference's literal divisors).
		// Everything is queued on the stream.  All frames have the channel count of the first.
		float* upload_as_f32(const std::vector<std::shared_ptr<const Audio_frame>>& frames, gpu::Pinned_buffer& h_raw, gpu::Device_buffer& d_raw,
							 gpu::Device_buffer& d_f32, size_t* total_samples)
		{
			nae_ctx* ctx = gpu::context();
			const int ch = frames.front()->data()->ch_layout.nb_channels;
			struct Place { size_t raw_off, stride, plane_bytes, out_off; int planes; bool wire; };
			std::vector<Place> place;
			size_t raw_bytes = 0, out_samples = 0;
			bool all_wire = true;
			for (const auto& f : frames)
			{
				const Frame_data* frame = f->data();
				const int bps = bytes_per_sample(frame->format);
				if (bps == 0 || frame->format == AV_SAMPLE_FMT_DBL)
					throw infra::Processor::Runtime_error(
						"Unsupported sample format", "The processors do not support the given sample format.",
						infra::fmt("Sample format: %d", frame->format)
					);
				const bool planar = sample_fmt_is_planar(frame->format);
				Place p;
				p.planes = planar ? ch : 1;
				p.plane_bytes = (size_t)frame->nb_samples * bps * (planar ? 1 : ch);
				p.wire = frame->format == AV_SAMPLE_FMT_FLT || (frame->format == AV_SAMPLE_FMT_FLTP && ch == 1);
				all_wire = all_wire && p.wire;
				// float planes lie back to back ([frame][ch][n]: what the strided interleave launch reads); integer planes start on 256 bytes
				const bool f32 = frame->format == AV_SAMPLE_FMT_FLT || frame->format == AV_SAMPLE_FMT_FLTP;
				p.stride = f32 ? p.plane_bytes : (p.plane_bytes + 255) / 256 * 256;
				raw_bytes = f32 ? (raw_bytes + 15) / 16 * 16 : (raw_bytes + 255) / 256 * 256;
				p.raw_off = raw_bytes;
				p.out_off = out_samples * ch;
				raw_bytes += p.stride * p.planes;
				out_samples += frame->nb_samples;
				place.push_back(p);
			}
			*total_samples = out_samples;
			auto* host = static_cast<uint8_t*>(h_raw.reserve(raw_bytes));
			float* out = static_cast<float*>(d_f32.reserve(out_samples * ch * sizeof(float)));
			if (all_wire)
			{
				// the staged bytes are the interleaved signal (offsets re-packed without the 16-byte rounding)
				size_t off = 0;
				for (size_t k = 0; k < frames.size(); k++)
				{
					std::memcpy(host + off, frames[k]->data()->data[0], place[k].plane_bytes);
					off += place[k].plane_bytes;
				}
				gpu::check(nae_memcpy_h2d(ctx, out, host, off), "h2d");
				return out;
			}
			auto* raw = static_cast<uint8_t*>(d_raw.reserve(raw_bytes));
			for (size_t k = 0; k < frames.size(); k++)
				for (int q = 0; q < place[k].planes; q++)
					std::memcpy(host + place[k].raw_off + q * place[k].stride, frames[k]->data()->data[q], place[k].plane_bytes);
			gpu::check(nae_memcpy_h2d(ctx, raw, host, raw_bytes), "h2d");
			for (size_t k = 0; k < frames.size();)
			{
				const Frame_data* frame = frames[k]->data();
				const Place& p = place[k];
				if (p.wire)
				{
					gpu::check(nae_memcpy_d2d(ctx, out + p.out_off, raw + p.raw_off, p.plane_bytes), "d2d");
					k++;
				}
				else if (frame->format == AV_SAMPLE_FMT_FLTP)
				{
					// run of planar stereo frames of this length, staged at a constant pitch
					const size_t n = (size_t)frame->nb_samples;
					size_t run = 1;
					while (k + run < frames.size() && frames[k + run]->data()->format == AV_SAMPLE_FMT_FLTP &&
						   (size_t)frames[k + run]->data()->nb_samples == n && place[k + run].raw_off == p.raw_off + run * (place[k + 1].raw_off - p.raw_off))
						run++;
					const size_t pitch_floats = run > 1 ? (place[k + 1].raw_off - p.raw_off) / sizeof(float) : 2 * n;
					const nae_sig src{raw + p.raw_off, pitch_floats, n, 1};
					const nae_sig dst{out + p.out_off, 2 * n, 1, 2};
					gpu::check(nae_copy_sig_f32(ctx, &src, &dst, n, 2, run), "nae_copy_sig_f32");
					k += run;
				}
				else
				{
					const void* pl[2] = {raw + p.raw_off, raw + p.raw_off + p.stride};
					gpu::check(nae_to_f32_interleaved(ctx, frame->format, pl, frame->nb_samples, ch, out + p.out_off), "nae_to_f32_interleaved");
					k++;
				}
			}
			return out;
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
			gpu::Node node;  // this node's context (own stream; device: gpu::pick_device): first local, destroyed last
			batch_stats = {};
			const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
			const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
			if (!input_item.has_value())
				throw infra::Processor::Runtime_error(
					processor_name + " has no input",
					processor_name + " requires an audio stream input to function properly.",
					"Input item 'input' not found"
				);
			Audio_stream& input_stream = input_item.value().get();
			Stretcher soundtouch;
			gpu::Device_buffer d_raw, d_f32, d_out;
			gpu::Pinned_buffer h_raw, h_out;
			bool input_stream_eof = false, pending_put = false;
			std::shared_ptr<const Audio_frame> held;  // popped, but with another channel count than the batch in front of it
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
					for (auto& stream : output_stream)
						while (!stop_token)
						{
							if (stream->try_push(new_frame) == channel_op_status::success) break;
							nae_fiber::this_fiber::yield();
						}
				}
			};

			while (!stop_token)
			{
				if (!input_stream_eof || held)
				{
					// Batching: the reference puts one frame per round; here every frame that is already waiting
					// (at most 16) is uploaded, converted and put as ONE block behind one wait.  The handle's output does not
					// depend on how its input is cut into puts (tests/test_gpu_stft.py, test_gpu_wsola.py: chunking invariance).
					constexpr size_t max_batch = 16;
					std::vector<std::shared_ptr<const Audio_frame>> batch;
					if (held) batch.push_back(std::move(held));
					held.reset();
					while (batch.size() < max_batch && !input_stream_eof)
					{
						const auto pop_result = input_stream.try_pop();
						if (!pop_result.has_value())
						{
							if (pop_result.error() != channel_op_status::empty)
								throw infra::Processor::Runtime_error(
									"Unexpected error when fetching audio frame", processor_name + " encountered an unexpected error.",
									infra::fmt("Channel fetch error: %d", (int)pop_result.error())
								);
							if (input_stream.eof()) input_stream_eof = true;
							break;
						}
						if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
						{
							held = pop_result.value();
							break;
						}
						batch.push_back(pop_result.value());
					}
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
			for (auto& stream : output_stream) stream->set_eof();
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
		const auto wrong = [](const char* field) {
			return Runtime_error(
				"Failed to deserialize JSON file",
				"Audio_spectrum failed to serialize the JSON input because of missing or invalid fields.",
				std::string("Wrong field: ") + field
			);
		};
		const auto integer = [&](const char* key, int fallback) {
			if (!value.isMember(key)) return fallback;  // no key: the default (a project saved before the key existed)
			const Json::Value& v = value[key];
			if (!v.isDouble() || v.asDouble() != (double)v.asInt()) throw wrong(key);
			return v.asInt();
		};
		const int n = integer("fft_size", default_fft_size), h = integer("hop", default_hop);
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
		gpu::Node node;  // this node's context (own stream): first local, destroyed last — before the handle guard and the buffers
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw Runtime_error("FFT Spectrum has no input", "FFT Spectrum requires an audio stream input to function properly.", "Input item 'input' not found");
		Audio_stream& input_stream = input_item.value().get();
		nae_ctx* ctx = gpu::context();
		last_context = ctx;
		nae_spectrum* spectrum = nullptr;
		struct Guard { nae_spectrum*& h; ~Guard() { if (h) nae_spectrum_destroy(h); } } guard{spectrum};
		gpu::Device_buffer d_raw, d_f32, d_out;
		gpu::Pinned_buffer h_raw, h_out;
		int ch = 0, sample_rate = 0;
		double time_seconds = 0.0;
		std::shared_ptr<const Audio_frame> held;  // popped, but with another channel count than the batch in front of it

		while (!stop_token)
		{
			// every frame that is already waiting (at most 16) is uploaded and put as one block behind one wait (the handle's
			// frames do not depend on how its input is cut into puts)
			constexpr size_t max_batch = 16;
			std::vector<std::shared_ptr<const Audio_frame>> batch;
			if (held) batch.push_back(std::move(held));
			held.reset();
			bool ended = false;
			while (batch.size() < max_batch)
			{
				const auto pop_result = input_stream.try_pop();
				if (!pop_result.has_value())
				{
					ended = input_stream.eof();
					break;
				}
				if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
				{
					held = pop_result.value();
					break;
				}
				batch.push_back(pop_result.value());
			}
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
				auto out = std::make_shared<Audio_frame>();
				Frame_data* o = out->data();
				o->format = AV_SAMPLE_FMT_FLTP;
				o->sample_rate = sample_rate;
				o->nb_samples = bins;
				o->ch_layout.nb_channels = ch;
				o->time_base = {1, 1000000};
				o->pts = (int64_t)(time_seconds * 1000000);
				frame_get_buffer(o, 32);
				for (int c = 0; c < ch; c++) std::memcpy(o->data[c], host + (f * ch + c) * bins, bins * sizeof(float));
				time_seconds += (double)hop / sample_rate;
				for (auto& stream : output_stream)
					while (!stop_token && stream->try_push(out) != channel_op_status::success) nae_fiber::this_fiber::yield();
			}
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// ------------------------------------------------------------------------------------------ Audio_filter
	namespace
	{
		const char* const kind_names[] = {"lowpass", "highpass", "bandpass", "bandstop"};
	}

	infra::Processor::Info Audio_filter::get_processor_info()
	{
		return {"audio_filter", "Audio Filter", false, [] { return std::unique_ptr<infra::Processor>(new Audio_filter); },
				"Linear-phase FIR low-pass / high-pass / band-pass / band-stop by FFT fast convolution (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_filter::get_pin_attributes() const
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	Json::Value Audio_filter::serialize() const
	{
		Json::Value value;
		if (kind != Kind::Lowpass) value["kind"] = kind_names[(int)kind];
		if (f_lo != default_f_lo) value["f_lo"] = f_lo;
		if (f_hi != default_f_hi) value["f_hi"] = f_hi;
		if (taps != default_taps) value["taps"] = taps;
		if (fft_size != 0) value["fft_size"] = fft_size;
		return value;
	}

	void Audio_filter::deserialize(const Json::Value& value)
	{
		const auto wrong = [](const char* field) {
			return Runtime_error(
				"Failed to deserialize JSON file",
				"Audio_filter failed to serialize the JSON input because of missing or invalid fields.",
				std::string("Wrong field: ") + field
			);
		};
		// everything is read and checked first: a rejected value leaves the node as it was
		Kind k = Kind::Lowpass;
		if (value.isMember("kind"))
		{
			int found = -1;
			if (value["kind"].isString())
				for (int i = 0; i < 4; i++)
					if (value["kind"].asString() == kind_names[i]) found = i;
			if (found < 0) throw wrong("kind");
			k = (Kind)found;
		}
		const auto hertz = [&](const char* key, float fallback) {
			if (!value.isMember(key)) return fallback;
			if (!value[key].isDouble() || !(value[key].asDouble() > 0.0 && value[key].asDouble() < 1e9)) throw wrong(key);
			return value[key].asFloat();
		};
		const float lo = hertz("f_lo", default_f_lo), hi = hertz("f_hi", default_f_hi);
		const auto integer = [&](const char* key, int fallback) {
			if (!value.isMember(key)) return fallback;
			const Json::Value& v = value[key];
			// compared as a double with the range first: a number outside int's range is never converted
			if (!v.isDouble() || !(v.asDouble() >= 1.0 && v.asDouble() <= 4096.0) || v.asDouble() != (double)v.asInt()) throw wrong(key);
			return v.asInt();
		};
		const int n_taps = integer("taps", default_taps);
		if (n_taps > max_taps || (n_taps & 1) == 0) throw wrong("taps");
		const int n_fft = integer("fft_size", 0);
		if (value.isMember("fft_size") && (nae_fir_pick_n_fft(n_fft / 2 + 1) != n_fft || n_taps > n_fft / 2 + 1)) throw wrong("fft_size");
		kind = k;
		f_lo = lo;
		f_hi = hi;
		taps = n_taps;
		fft_size = n_fft;
	}

	void Audio_filter::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // this node's context (own stream): first local, destroyed last — before the handle guard and the buffers
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw Runtime_error("Audio Filter has no input", "Audio Filter requires an audio stream input to function properly.", "Input item 'input' not found");
		Audio_stream& input_stream = input_item.value().get();
		nae_ctx* ctx = gpu::context();
		nae_fir* fir = nullptr;
		struct Guard { nae_fir*& h; ~Guard() { if (h) nae_fir_destroy(h); } } guard{fir};
		gpu::Device_buffer d_raw, d_f32, d_out;
		gpu::Pinned_buffer h_raw, h_out;
		int ch = 0;
		size_t to_discard = (size_t)(taps - 1) / 2;  // the group delay
		struct Shape { int nb_samples, sample_rate; int64_t pts; decltype(Frame_data::time_base) time_base; };
		std::deque<Shape> shapes;     // the input frames whose output is still owed
		std::vector<float> ready;     // filtered samples behind the group delay, interleaved, not yet cut into frames
		size_t ready_pos = 0;         // frames of `ready` already delivered
		std::shared_ptr<const Audio_frame> held;  // popped, but with another channel count than the batch in front of it

		// everything the handle has ready comes down behind ONE wait and leaves as frames of the input's sizes
		const auto deliver = [&]()
		{
			const size_t avail = nae_fir_available(fir);
			if (avail == 0) { gpu::wait(stop_token); return; }
			float* dev = static_cast<float*>(d_out.reserve(avail * ch * sizeof(float)));
			float* host = static_cast<float*>(h_out.reserve(avail * ch * sizeof(float)));
			size_t got = 0;
			gpu::check(nae_fir_receive(fir, dev, avail, &got), "nae_fir_receive");
			gpu::check(nae_memcpy_d2h(ctx, host, dev, got * ch * sizeof(float)), "d2h");
			gpu::wait(stop_token);
			const size_t skip = std::min(to_discard, got);
			to_discard -= skip;
			ready.erase(ready.begin(), ready.begin() + ready_pos * ch);
			ready_pos = 0;
			ready.insert(ready.end(), host + skip * ch, host + got * ch);
			while (!shapes.empty() && !stop_token && ready.size() / ch - ready_pos >= (size_t)shapes.front().nb_samples)
			{
				const Shape s = shapes.front();
				shapes.pop_front();
				auto out = std::make_shared<Audio_frame>();
				Frame_data* o = out->data();
				o->format = AV_SAMPLE_FMT_FLT;
				o->sample_rate = s.sample_rate;
				o->nb_samples = s.nb_samples;
				o->ch_layout.nb_channels = ch;
				o->time_base = s.time_base;
				o->pts = s.pts;
				frame_get_buffer(o, 32);
				std::memcpy(o->data[0], ready.data() + ready_pos * ch, (size_t)s.nb_samples * ch * sizeof(float));
				ready_pos += s.nb_samples;
				for (auto& stream : output_stream)
					while (!stop_token && stream->try_push(out) != channel_op_status::success) nae_fiber::this_fiber::yield();
			}
		};

		while (!stop_token)
		{
			// every frame that is already waiting (at most 16) is uploaded and put as one block (the handle's output does not depend on how
			// its input is cut into puts)
			constexpr size_t max_batch = 16;
			std::vector<std::shared_ptr<const Audio_frame>> batch;
			if (held) batch.push_back(std::move(held));
			held.reset();
			bool ended = false;
			while (batch.size() < max_batch)
			{
				const auto pop_result = input_stream.try_pop();
				if (!pop_result.has_value())
				{
					ended = input_stream.eof();
					break;
				}
				if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
				{
					held = pop_result.value();
					break;
				}
				batch.push_back(pop_result.value());
			}
			if (batch.empty())
			{
				if (!ended)
				{
					nae_fiber::this_fiber::yield();
					continue;
				}
				if (fir != nullptr)
				{
					// the tail: (L - 1) / 2 of the L - 1 flushed frames complete the frames still owed
					gpu::check(nae_fir_flush(fir), "nae_fir_flush");
					deliver();
				}
				break;
			}
			const Frame_data* frame = batch.front()->data();
			if (fir == nullptr)
			{
				ch = frame->ch_layout.nb_channels;
				if (ch != 1 && ch != 2) throw Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels", ch));
				std::vector<float> h((size_t)taps);
				if (nae_fir_design((int)kind, frame->sample_rate, f_lo, f_hi, taps, h.data()) != NAE_OK)
					throw Runtime_error(
						"Invalid filter frequencies", "The filter's corner frequencies must lie below half of the sample rate, the lower below the upper.",
						infra::fmt("f_lo %g Hz, f_hi %g Hz at %d Hz", (double)f_lo, (double)f_hi, frame->sample_rate)
					);
				gpu::check(nae_fir_create(ctx, h.data(), taps, fft_size, ch, &fir), "nae_fir_create");
			}
			else if (frame->ch_layout.nb_channels != ch)
				throw Runtime_error("Channel count changed", "The filter runs one stream of a fixed channel count.",
									infra::fmt("Got %d channels after %d", frame->ch_layout.nb_channels, ch));
			for (const auto& f : batch) shapes.push_back({f->data()->nb_samples, f->data()->sample_rate, f->data()->pts, f->data()->time_base});
			size_t total = 0;
			float* samples = upload_as_f32(batch, h_raw, d_raw, d_f32, &total);
			gpu::check(nae_fir_put(fir, samples, total), "nae_fir_put");
			deliver();
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// ------------------------------------------------------------------------------------------ Audio_reverb
	infra::Processor::Info Audio_reverb::get_processor_info()
	{
		return {"audio_reverb", "Audio Reverb", false, [] { return std::unique_ptr<infra::Processor>(new Audio_reverb); },
				"Convolution reverb with a designed, per-channel decaying-noise response by partitioned FFT convolution (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_reverb::get_pin_attributes() const
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	Json::Value Audio_reverb::serialize() const
	{
		Json::Value value;
		if (rt60 != default_rt60) value["rt60"] = rt60;
		if (predelay_ms != default_predelay_ms) value["predelay_ms"] = predelay_ms;
		if (wet != default_wet) value["wet"] = wet;
		if (dry != default_dry) value["dry"] = dry;
		if (seed != 1) value["seed"] = (double)seed;   // below 2^53 (deserialize): exact
		if (fft_size != 0) value["fft_size"] = fft_size;
		return value;
	}

	void Audio_reverb::deserialize(const Json::Value& value)
	{
		const auto wrong = [](const char* field) {
			return Runtime_error(
				"Failed to deserialize JSON file",
				"Audio_reverb failed to serialize the JSON input because of missing or invalid fields.",
				std::string("Wrong field: ") + field
			);
		};
		// everything is read and checked first: a rejected value leaves the node as it was
		const auto real = [&](const char* key, double lo, double hi, double fallback) {
			if (!value.isMember(key)) return fallback;
			if (!value[key].isDouble() || !(value[key].asDouble() >= lo && value[key].asDouble() <= hi)) throw wrong(key);
			return value[key].asDouble();
		};
		const double r = real("rt60", 0.1, 5.0, default_rt60), p = real("predelay_ms", 0.0, 200.0, default_predelay_ms);
		const double w = real("wet", 0.0, 1.0, default_wet), d = real("dry", 0.0, 1.0, default_dry);
		uint64_t sd = 1;
		if (value.isMember("seed"))
		{
			// compared as a double with the range first: a number outside the integer range is never converted
			const Json::Value& v = value["seed"];
			if (!v.isDouble() || !(v.asDouble() >= 0.0 && v.asDouble() < 9007199254740992.0) || v.asDouble() != (double)(uint64_t)v.asDouble()) throw wrong("seed");
			sd = (uint64_t)v.asDouble();
		}
		int n_fft = 0;
		if (value.isMember("fft_size"))
		{
			const Json::Value& v = value["fft_size"];
			if (!v.isDouble() || !(v.asDouble() >= 1.0 && v.asDouble() <= 4096.0) || v.asDouble() != (double)v.asInt()) throw wrong("fft_size");
			n_fft = v.asInt();
			if (nae_fir_pick_n_fft(n_fft / 2 + 1) != n_fft) throw wrong("fft_size");   // the filter's sizes: 512, 1024, 2048, 4096
		}
		rt60 = r;
		predelay_ms = p;
		wet = w;
		dry = d;
		seed = sd;
		fft_size = n_fft;
	}

	void Audio_reverb::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // this node's context (own stream): first local, destroyed last — before the handle guard and the buffers
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw Runtime_error("Audio Reverb has no input", "Audio Reverb requires an audio stream input to function properly.", "Input item 'input' not found");
		Audio_stream& input_stream = input_item.value().get();
		nae_ctx* ctx = gpu::context();
		nae_conv* conv = nullptr;
		struct Guard { nae_conv*& h; ~Guard() { if (h) nae_conv_destroy(h); } } guard{conv};
		gpu::Device_buffer d_raw, d_f32, d_out;
		gpu::Pinned_buffer h_raw, h_out;
		int ch = 0;
		struct Shape { int nb_samples, sample_rate; int64_t pts; decltype(Frame_data::time_base) time_base; };
		std::deque<Shape> shapes;     // the input frames whose output is still owed
		std::vector<float> ready;     // convolved samples, interleaved, not yet cut into frames
		size_t ready_pos = 0;         // frames of `ready` already delivered
		std::shared_ptr<const Audio_frame> held;  // popped, but with another channel count than the batch in front of it

		// everything the handle has ready comes down behind ONE wait and leaves as frames of the input's sizes
		const auto deliver = [&]()
		{
			const size_t avail = nae_conv_available(conv);
			if (avail == 0) { gpu::wait(stop_token); return; }
			float* dev = static_cast<float*>(d_out.reserve(avail * ch * sizeof(float)));
			float* host = static_cast<float*>(h_out.reserve(avail * ch * sizeof(float)));
			size_t got = 0;
			gpu::check(nae_conv_receive(conv, dev, avail, &got), "nae_conv_receive");
			gpu::check(nae_memcpy_d2h(ctx, host, dev, got * ch * sizeof(float)), "d2h");
			gpu::wait(stop_token);
			ready.erase(ready.begin(), ready.begin() + ready_pos * ch);
			ready_pos = 0;
			ready.insert(ready.end(), host, host + got * ch);
			while (!shapes.empty() && !stop_token && ready.size() / ch - ready_pos >= (size_t)shapes.front().nb_samples)
			{
				const Shape s = shapes.front();
				shapes.pop_front();
				auto out = std::make_shared<Audio_frame>();
				Frame_data* o = out->data();
				o->format = AV_SAMPLE_FMT_FLT;
				o->sample_rate = s.sample_rate;
				o->nb_samples = s.nb_samples;
				o->ch_layout.nb_channels = ch;
				o->time_base = s.time_base;
				o->pts = s.pts;
				frame_get_buffer(o, 32);
				std::memcpy(o->data[0], ready.data() + ready_pos * ch, (size_t)s.nb_samples * ch * sizeof(float));
				ready_pos += s.nb_samples;
				for (auto& stream : output_stream)
					while (!stop_token && stream->try_push(out) != channel_op_status::success) nae_fiber::this_fiber::yield();
			}
		};

		while (!stop_token)
		{
			constexpr size_t max_batch = 16;   // as the filter node: every frame that is already waiting is put as one block
			std::vector<std::shared_ptr<const Audio_frame>> batch;
			if (held) batch.push_back(std::move(held));
			held.reset();
			bool ended = false;
			while (batch.size() < max_batch)
			{
				const auto pop_result = input_stream.try_pop();
				if (!pop_result.has_value())
				{
					ended = input_stream.eof();
					break;
				}
				if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
				{
					held = pop_result.value();
					break;
				}
				batch.push_back(pop_result.value());
			}
			if (batch.empty())
			{
				if (!ended)
				{
					nae_fiber::this_fiber::yield();
					continue;
				}
				if (conv != nullptr)
				{
					// the last partial block comes out with the flush; the frames still owed are cut from it and the tail behind them is dropped
					gpu::check(nae_conv_flush(conv), "nae_conv_flush");
					deliver();
				}
				break;
			}
			const Frame_data* frame = batch.front()->data();
			if (conv == nullptr)
			{
				ch = frame->ch_layout.nb_channels;
				if (ch != 1 && ch != 2) throw Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels", ch));
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
				gpu::check(nae_conv_create(ctx, h.data(), n_taps, ch, fft_size, ch, &conv), "nae_conv_create");
			}
			else if (frame->ch_layout.nb_channels != ch)
				throw Runtime_error("Channel count changed", "The reverb runs one stream of a fixed channel count.",
									infra::fmt("Got %d channels after %d", frame->ch_layout.nb_channels, ch));
			for (const auto& f : batch) shapes.push_back({f->data()->nb_samples, f->data()->sample_rate, f->data()->pts, f->data()->time_base});
			size_t total = 0;
			float* samples = upload_as_f32(batch, h_raw, d_raw, d_f32, &total);
			gpu::check(nae_conv_put(conv, samples, total), "nae_conv_put");
			deliver();
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// What the nodes on a compensated streaming handle share (the equalizer, the dynamics node): frames are put as they come, in batches;
	// everything the handle has ready leaves as frames of the input's sizes, pts and time base; the flush at the end of the stream releases
	// the rest.  `create` makes the handle from the first frame (its sample rate) and the channel count, or throws.
	template <class Handle>
	struct Handle_ops
	{
		int (*put)(Handle*, const float*, size_t);
		int (*flush)(Handle*);
		size_t (*available)(Handle*);
		int (*receive)(Handle*, float*, size_t, size_t*);
		int (*destroy)(Handle*);
	};

	template <class Handle, class Create>
	static void run_on_handle(
		Audio_stream& input_stream, const std::set<std::shared_ptr<Audio_stream>>& output_stream, const std::atomic<bool>& stop_token,
		const std::type_identity_t<Handle_ops<Handle>>& ops, const Create& create
	)
	{
		nae_ctx* ctx = gpu::context();
		Handle* h = nullptr;
		struct Guard { Handle*& h; int (*destroy)(Handle*); ~Guard() { if (h) destroy(h); } } guard{h, ops.destroy};
		gpu::Device_buffer d_raw, d_f32, d_out;
		gpu::Pinned_buffer h_raw, h_out;
		int ch = 0;
		struct Shape { int nb_samples, sample_rate; int64_t pts; decltype(Frame_data::time_base) time_base; };
		std::deque<Shape> shapes;     // the input frames whose output is still owed
		std::vector<float> ready;     // filtered samples, interleaved, not yet cut into frames
		size_t ready_pos = 0;         // frames of `ready` already delivered
		std::shared_ptr<const Audio_frame> held;  // popped, but with another channel count than the batch in front of it

		// everything the handle has ready comes down behind ONE wait and leaves as frames of the input's sizes
		const auto deliver = [&]()
		{
			const size_t avail = ops.available(h);
			if (avail == 0) { gpu::wait(stop_token); return; }
			float* dev = static_cast<float*>(d_out.reserve(avail * ch * sizeof(float)));
			float* host = static_cast<float*>(h_out.reserve(avail * ch * sizeof(float)));
			size_t got = 0;
			gpu::check(ops.receive(h, dev, avail, &got), "receive");
			gpu::check(nae_memcpy_d2h(ctx, host, dev, got * ch * sizeof(float)), "d2h");
			gpu::wait(stop_token);
			ready.erase(ready.begin(), ready.begin() + ready_pos * ch);
			ready_pos = 0;
			ready.insert(ready.end(), host, host + got * ch);
			while (!shapes.empty() && !stop_token && ready.size() / ch - ready_pos >= (size_t)shapes.front().nb_samples)
			{
				const Shape s = shapes.front();
				shapes.pop_front();
				auto out = std::make_shared<Audio_frame>();
				Frame_data* o = out->data();
				o->format = AV_SAMPLE_FMT_FLT;
				o->sample_rate = s.sample_rate;
				o->nb_samples = s.nb_samples;
				o->ch_layout.nb_channels = ch;
				o->time_base = s.time_base;
				o->pts = s.pts;
				frame_get_buffer(o, 32);
				std::memcpy(o->data[0], ready.data() + ready_pos * ch, (size_t)s.nb_samples * ch * sizeof(float));
				ready_pos += s.nb_samples;
				for (auto& stream : output_stream)
					while (!stop_token && stream->try_push(out) != channel_op_status::success) nae_fiber::this_fiber::yield();
			}
		};

		while (!stop_token)
		{
			constexpr size_t max_batch = 16;   // as the filter node: every frame that is already waiting is put as one block
			std::vector<std::shared_ptr<const Audio_frame>> batch;
			if (held) batch.push_back(std::move(held));
			held.reset();
			bool ended = false;
			while (batch.size() < max_batch)
			{
				const auto pop_result = input_stream.try_pop();
				if (!pop_result.has_value())
				{
					ended = input_stream.eof();
					break;
				}
				if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
				{
					held = pop_result.value();
					break;
				}
				batch.push_back(pop_result.value());
			}
			if (batch.empty())
			{
				if (!ended)
				{
					nae_fiber::this_fiber::yield();
					continue;
				}
				if (h != nullptr)
				{
					// what the handle still holds comes out with the flush: every frame still owed is complete
					gpu::check(ops.flush(h), "flush");
					deliver();
				}
				break;
			}
			const Frame_data* frame = batch.front()->data();
			if (h == nullptr)
			{
				ch = frame->ch_layout.nb_channels;
				if (ch != 1 && ch != 2) throw infra::Processor::Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels", ch));
				h = create(ctx, frame, ch);
			}
			else if (frame->ch_layout.nb_channels != ch)
				throw infra::Processor::Runtime_error("Channel count changed", "The node runs one stream of a fixed channel count.",
									infra::fmt("Got %d channels after %d", frame->ch_layout.nb_channels, ch));
			for (const auto& f : batch) shapes.push_back({f->data()->nb_samples, f->data()->sample_rate, f->data()->pts, f->data()->time_base});
			size_t total = 0;
			float* samples = upload_as_f32(batch, h_raw, d_raw, d_f32, &total);
			gpu::check(ops.put(h, samples, total), "put");
			deliver();
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// ------------------------------------------------------------------------------------------ Audio_eq
	infra::Processor::Info Audio_eq::get_processor_info()
	{
		return {"audio_eq", "Audio Equalizer", false, [] { return std::unique_ptr<infra::Processor>(new Audio_eq); },
				"Parametric equalizer: up to 16 peaking, shelving, low-pass, high-pass and notch bands as a biquad cascade in double (MI355X)"};
	}

	std::vector<infra::Processor::Pin_attribute> Audio_eq::get_pin_attributes() const
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	static const char* const eq_kind_names[] = {"peak", "lowshelf", "highshelf", "lowpass", "highpass", "notch"};

	Json::Value Audio_eq::serialize() const
	{
		Json::Value value;
		if (bands.empty()) return value;
		Json::Value list(Json::arrayValue);
		for (const Band& b : bands)
		{
			Json::Value v;
			if (b.kind != Kind::Peak) v["kind"] = eq_kind_names[(int)b.kind];
			if (b.freq != Band::default_freq) v["freq"] = b.freq;
			if (b.gain_db != Band::default_gain_db) v["gain_db"] = b.gain_db;
			if (b.q != Band::default_q) v["q"] = b.q;
			list.append(v);
		}
		value["bands"] = list;
		return value;
	}

	void Audio_eq::deserialize(const Json::Value& value)
	{
		const auto wrong = [](const char* field) {
			return Runtime_error(
				"Failed to deserialize JSON file",
				"Audio_eq failed to serialize the JSON input because of missing or invalid fields.",
				std::string("Wrong field: ") + field
			);
		};
		// everything is read and checked first: a rejected value leaves the node as it was
		std::vector<Band> read;
		if (value.isMember("bands"))
		{
			const Json::Value& list = value["bands"];
			if (!list.isArray() || list.size() > max_bands) throw wrong("bands");
			for (int i = 0; i < (int)list.size(); i++)
			{
				const Json::Value& v = list[i];
				if (v.isArray() || v.isDouble() || v.isBool() || v.isString()) throw wrong("bands");   // an object, possibly without a key
				Band b;
				if (v.isMember("kind"))
				{
					if (!v["kind"].isString()) throw wrong("kind");
					int k = 0;
					while (k < 6 && v["kind"].asString() != eq_kind_names[k]) k++;
					if (k == 6) throw wrong("kind");
					b.kind = (Kind)k;
				}
				const auto real = [&](const char* key, double lo, double hi, double fallback) {
					if (!v.isMember(key)) return fallback;
					if (!v[key].isDouble() || !(v[key].asDouble() >= lo && v[key].asDouble() <= hi)) throw wrong(key);
					return v[key].asDouble();
				};
				b.freq = real("freq", 0.0, 1e9, Band::default_freq);
				if (!(b.freq > 0.0)) throw wrong("freq");
				b.gain_db = real("gain_db", -24.0, 24.0, Band::default_gain_db);
				b.q = real("q", 0.1, 40.0, Band::default_q);
				read.push_back(b);
			}
		}
		bands = std::move(read);
	}

	void Audio_eq::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // this node's context (own stream): first local, destroyed last — before the handle guard and the buffers
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw Runtime_error("Audio Equalizer has no input", "Audio Equalizer requires an audio stream input to function properly.", "Input item 'input' not found");
		Audio_stream& input_stream = input_item.value().get();
		if (bands.empty())
		{
			// a wire: the frames pass as they are
			while (!stop_token)
			{
				const auto pop_result = input_stream.try_pop();
				if (!pop_result.has_value())
				{
					if (input_stream.eof()) break;
					nae_fiber::this_fiber::yield();
					continue;
				}
				for (auto& stream : output_stream)
					while (!stop_token && stream->try_push(pop_result.value()) != channel_op_status::success) nae_fiber::this_fiber::yield();
			}
			for (auto& stream : output_stream) stream->set_eof();
			return;
		}
		run_on_handle<nae_eq>(
			input_stream, output_stream, stop_token, {nae_eq_put, nae_eq_flush, nae_eq_available, nae_eq_receive, nae_eq_destroy},
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				std::vector<double> coef(bands.size() * 5);
				for (size_t i = 0; i < bands.size(); i++)
					if (nae_eq_design((int)bands[i].kind, frame->sample_rate, bands[i].freq, bands[i].gain_db, bands[i].q, coef.data() + 5 * i) != NAE_OK)
						throw Runtime_error("Invalid equalizer band", "A band's frequency must lie below half the stream's sample rate.",
											infra::fmt("band %d: %g Hz at %d Hz", (int)i, bands[i].freq, frame->sample_rate));
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

	std::vector<infra::Processor::Pin_attribute> Audio_dynamics::get_pin_attributes() const
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	Json::Value Audio_dynamics::serialize() const
	{
		Json::Value value;
		if (mode != Mode::Compressor) value["mode"] = "limiter";
		if (threshold_db != default_threshold_db) value["threshold_db"] = threshold_db;
		if (ratio != default_ratio) value["ratio"] = ratio;
		if (knee_db != default_knee_db) value["knee_db"] = knee_db;
		if (attack_ms != default_attack_ms) value["attack_ms"] = attack_ms;
		if (release_ms != default_release_ms) value["release_ms"] = release_ms;
		if (lookahead_ms != default_lookahead_ms) value["lookahead_ms"] = lookahead_ms;
		if (makeup_db != default_makeup_db) value["makeup_db"] = makeup_db;
		if (!link_channels) value["link_channels"] = false;
		return value;
	}

	void Audio_dynamics::deserialize(const Json::Value& value)
	{
		const auto wrong = [](const char* field) {
			return Runtime_error(
				"Failed to deserialize JSON file",
				"Audio_dynamics failed to serialize the JSON input because of missing or invalid fields.",
				std::string("Wrong field: ") + field
			);
		};
		// everything is read and checked first: a rejected value leaves the node as it was; an absent key is its default
		Mode m = Mode::Compressor;
		if (value.isMember("mode"))
		{
			if (!value["mode"].isString()) throw wrong("mode");
			const std::string name = value["mode"].asString();
			if (name == "limiter") m = Mode::Limiter;
			else if (name != "compressor") throw wrong("mode");
		}
		const auto real = [&](const char* key, double lo, double hi, double fallback) {
			if (!value.isMember(key)) return fallback;
			if (!value[key].isDouble() || !(value[key].asDouble() >= lo && value[key].asDouble() <= hi)) throw wrong(key);
			return value[key].asDouble();
		};
		const double t = real("threshold_db", -60.0, 0.0, default_threshold_db);
		const double r = real("ratio", 1.0, 100.0, default_ratio);
		const double k = real("knee_db", 0.0, 24.0, default_knee_db);
		const double a = real("attack_ms", 0.0, 500.0, default_attack_ms);
		const double rl = real("release_ms", 1.0, 5000.0, default_release_ms);
		const double la = real("lookahead_ms", 0.0, 20.0, default_lookahead_ms);
		const double mk = real("makeup_db", -24.0, 24.0, default_makeup_db);
		bool link = true;
		if (value.isMember("link_channels"))
		{
			if (!value["link_channels"].isBool()) throw wrong("link_channels");
			link = value["link_channels"].asBool();
		}
		mode = m;
		threshold_db = t; ratio = r; knee_db = k; attack_ms = a; release_ms = rl; lookahead_ms = la; makeup_db = mk;
		link_channels = link;
	}

	void Audio_dynamics::process_payload(
		const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
		const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
		const std::atomic<bool>& stop_token, std::any&
	)
	{
		gpu::Node node;  // this node's context (own stream): first local, destroyed last — before the handle guard and the buffers
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		const auto output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw Runtime_error("Audio Dynamics has no input", "Audio Dynamics requires an audio stream input to function properly.", "Input item 'input' not found");
		Audio_stream& input_stream = input_item.value().get();
		run_on_handle<nae_dyn>(
			input_stream, output_stream, stop_token, {nae_dyn_put, nae_dyn_flush, nae_dyn_available, nae_dyn_receive, nae_dyn_destroy},
			[&](nae_ctx* ctx, const Frame_data* frame, int ch)
			{
				nae_dyn_params params;
				const int rc = nae_dyn_design(frame->sample_rate, threshold_db, mode == Mode::Limiter ? INFINITY : ratio, knee_db, attack_ms / 1000.0,
											  release_ms / 1000.0, lookahead_ms / 1000.0, makeup_db, link_channels ? 1 : 0, &params);
				if (rc == NAE_ERR_UNSUPPORTED)
					throw Runtime_error("Look-ahead too long", "The look-ahead must not exceed 1024 samples at the stream's sample rate.",
										infra::fmt("lookahead %g ms at %d Hz", lookahead_ms, frame->sample_rate));
				if (rc != NAE_OK)
					throw Runtime_error("Invalid dynamics parameters", "A parameter of the dynamics node lies outside its range.",
										infra::fmt("nae_dyn_design at %d Hz: code %d", frame->sample_rate, rc));
				nae_dyn* dyn = nullptr;
				gpu::check(nae_dyn_create(ctx, &params, ch, &dyn), "nae_dyn_create");
				return dyn;
			}
		);
	}
}
