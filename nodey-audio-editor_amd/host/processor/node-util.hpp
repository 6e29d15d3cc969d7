// processor/node-util.hpp — what the nodes of audio-velocity.cpp and audio-effects.cpp share (not part of the plugin interface): the pins, the
// JSON field readers and their error, the collection of a batch of waiting frames and its upload as interleaved f32.
#pragma once
#include "audio-stream.hpp"
#include "gpu-context.hpp"

#include <cstring>
#include <string>
#include <vector>

namespace processor::detail
{
	inline std::vector<infra::Processor::Pin_attribute> io_pins()
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	// the error of a JSON field of the wrong type or outside its range
	inline infra::Processor::Runtime_error wrong_field(const char* node_name, const char* field)
	{
		return infra::Processor::Runtime_error(
			"Failed to deserialize JSON file",
			std::string(node_name) + " failed to serialize the JSON input because of missing or invalid fields.",
			std::string("Wrong field: ") + field
		);
	}

	// an optional bool: no key is false, a value that is not a bool is the wrong field
	inline bool bool_from_json(const Json::Value& value, const char* node_name, const char* key)
	{
		if (!value.isMember(key)) return false;
		if (!value[key].isBool()) throw wrong_field(node_name, key);
		return value[key].asBool();
	}

	// an optional number in [lo, hi]: no key is the fallback
	inline double real_from_json(const Json::Value& value, const char* node_name, const char* key, double lo, double hi, double fallback)
	{
		if (!value.isMember(key)) return fallback;
		if (!value[key].isDouble() || !(value[key].asDouble() >= lo && value[key].asDouble() <= hi)) throw wrong_field(node_name, key);
		return value[key].asDouble();
	}

	// Every frame that is already waiting, at most 16: a node uploads and puts them as ONE block behind one wait (a handle's output does not
	// depend on how its input is cut into puts).  A frame of another channel count than the batch in front of it is held back for the next
	// call.  *ended: the stream had nothing more and is at its end.
	inline std::vector<std::shared_ptr<const Audio_frame>> collect_batch(Audio_stream& input_stream, std::shared_ptr<const Audio_frame>& held, bool* ended)
	{
		constexpr size_t max_batch = 16;
		std::vector<std::shared_ptr<const Audio_frame>> batch;
		if (held) batch.push_back(std::move(held));
		held.reset();
		*ended = false;
		while (batch.size() < max_batch)
		{
			const auto pop_result = input_stream.try_pop();
			if (!pop_result.has_value())
			{
				*ended = input_stream.eof();
				break;
			}
			if (!batch.empty() && pop_result.value()->data()->ch_layout.nb_channels != batch.front()->data()->ch_layout.nb_channels)
			{
				held = pop_result.value();
				break;
			}
			batch.push_back(pop_result.value());
		}
		return batch;
	}

	// frames -> device interleaved f32, one after the other (extract_samples_interleaved, :150-232).  The frames of a batch are
	// copied into page-locked staging on the CPU and go up as ONE asynchronous copy; on the device
	//   * packed float frames (and mono planar ones) already ARE the interleaved signal: no kernel at all;
	//   * a run of planar stereo float frames of equal length is interleaved by ONE strided launch (frames as "streams");
	//   * integer formats: nae_to_f32_interleaved per frame (the reference's literal divisors).
	// Everything is queued on the stream.  All frames have the channel count of the first.
	inline float* upload_as_f32(const std::vector<std::shared_ptr<const Audio_frame>>& frames, gpu::Pinned_buffer& h_raw, gpu::Device_buffer& d_raw,
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
}
