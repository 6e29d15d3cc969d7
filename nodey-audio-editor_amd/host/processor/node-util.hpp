// processor/node-util.hpp — what the nodes of audio-velocity.cpp and audio-effects.cpp share (not part of the plugin interface), each piece
// written once: the pins and the node's streams (node_streams, with the "has no input" error), the JSON field readers and their error (a node
// does not call them key by key: it states its parameters as one list of fields, node-fields.hpp, which stands on these readers), the way
// out (push_to_all, make_f32_frame, pass_through), the collection of a batch of waiting frames and its upload as interleaved f32, and the two
// ends of a node that sits on a handle: take_in (frames in, held until enough have come) and cut_and_push (f32 out, as frames of the input's shapes).
#pragma once
#include "audio-stream.hpp"
#include "gpu-context.hpp"

#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace processor::detail
{
	using Frame_ptr = std::shared_ptr<const Audio_frame>;
	using Output_streams = std::set<std::shared_ptr<Audio_stream>>;
	using Time_base = decltype(Frame_data::time_base);

	inline std::vector<infra::Processor::Pin_attribute> io_pins()
	{
		return {
			{"output", "Output", typeid(Audio_stream), false, [] { return std::make_shared<Audio_stream>(); }},
			{"input", "Input", typeid(Audio_stream), true, [] { return std::make_shared<Audio_stream>(); }}
		};
	}

	// the stream on the node's "input" pin and every stream on its "output" pin; a node without an input is the user's error, under its display name
	struct Node_streams { Audio_stream& input; Output_streams output; };
	inline Node_streams node_streams(const infra::Processor::Input_map& input, const infra::Processor::Output_map& output, const std::string& display_name)
	{
		const auto input_item = infra::get_input_item<Audio_stream>(input, "input");
		Output_streams output_stream = infra::get_output_item<Audio_stream>(output, "output");
		if (!input_item.has_value())
			throw infra::Processor::Runtime_error(
				display_name + " has no input", display_name + " requires an audio stream input to function properly.", "Input item 'input' not found"
			);
		return {input_item.value().get(), std::move(output_stream)};
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

	// an optional bool: no key is the fallback, a value that is not a bool is the wrong field
	inline bool bool_from_json(const Json::Value& value, const char* node_name, const char* key, bool fallback = false)
	{
		if (!value.isMember(key)) return fallback;
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

	// an optional integer in [lo, hi]: no key is the fallback.  Compared as a double with the range first: a number outside int's range is never
	// converted
	inline int int_from_json(const Json::Value& value, const char* node_name, const char* key, int lo, int hi, int fallback)
	{
		if (!value.isMember(key)) return fallback;
		const Json::Value& v = value[key];
		if (!v.isDouble() || !(v.asDouble() >= (double)lo && v.asDouble() <= (double)hi) || v.asDouble() != (double)v.asInt()) throw wrong_field(node_name, key);
		return v.asInt();
	}

	// the frame goes to every output stream; a full stream is waited for, yielding, unless the run is stopped
	inline void push_to_all(const Output_streams& output_stream, const Frame_ptr& frame, const std::atomic<bool>& stop_token)
	{
		for (auto& stream : output_stream)
			while (!stop_token && stream->try_push(frame) != channel_op_status::success) nae_fiber::this_fiber::yield();
	}

	// a float frame of n samples of ch channels: packed (AV_SAMPLE_FMT_FLT) from interleaved samples, or planar (AV_SAMPLE_FMT_FLTP) from ch planes
	// of n floats back to back
	inline std::shared_ptr<Audio_frame> make_f32_frame(const float* samples, int n, int ch, int sample_rate, int64_t pts, Time_base time_base, bool planar = false)
	{
		auto out = std::make_shared<Audio_frame>();
		Frame_data* o = out->data();
		o->format = planar ? AV_SAMPLE_FMT_FLTP : AV_SAMPLE_FMT_FLT;
		o->sample_rate = sample_rate;
		o->nb_samples = n;
		o->ch_layout.nb_channels = ch;
		o->time_base = time_base;
		o->pts = pts;
		frame_get_buffer(o, 32);
		const int planes = planar ? ch : 1;
		for (int p = 0; p < planes; p++) std::memcpy(o->data[p], samples + (size_t)p * n, (size_t)n * (ch / planes) * sizeof(float));
		return out;
	}

	// a wire: the frames pass as they are, then the end of the stream
	inline void pass_through(Audio_stream& input_stream, const Output_streams& output_stream, const std::atomic<bool>& stop_token)
	{
		while (!stop_token)
		{
			const auto pop_result = input_stream.try_pop();
			if (pop_result.has_value()) push_to_all(output_stream, pop_result.value(), stop_token);
			else if (input_stream.eof()) break;
			else nae_fiber::this_fiber::yield();
		}
		for (auto& stream : output_stream) stream->set_eof();
	}

	// Every frame that is already waiting, at most 16: a node uploads and puts them as ONE block behind one wait (a handle's output does not
	// depend on how its input is cut into puts).  A frame of another channel count than the batch in front of it is held back for the next
	// call.  *ended: the stream had nothing more and is at its end.
	inline std::vector<Frame_ptr> collect_batch(Audio_stream& input_stream, Frame_ptr& held, bool* ended)
	{
		constexpr size_t max_batch = 16;
		std::vector<Frame_ptr> batch;
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
	inline float* upload_as_f32(const std::vector<Frame_ptr>& frames, gpu::Pinned_buffer& h_raw, gpu::Device_buffer& d_raw,
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

	// The intake of a node that sits on a handle.  The frames of one stream of a fixed channel count come in by batches and wait in `pending`
	// until the node puts them: at once when its handle exists, else when `need` samples have arrived (hold(first frame) says how many the
	// handle is made from) or the stream has ended.  Every frame taken in leaves its shape behind: the output is cut into frames of these.
	struct Shape { int nb_samples, sample_rate; int64_t pts; Time_base time_base; };
	struct Intake
	{
		int ch = 0;                       // the stream's channel count: the first frame's
		std::deque<Shape> shapes;         // the frames taken in whose output is still owed
		std::vector<Frame_ptr> pending;   // frames not yet put
		size_t pending_samples = 0, need = 0;
		bool at_end = false;              // nothing waited and the stream is at its end
		Frame_ptr held;                   // popped, but with another channel count than the batch in front of it
	};

	// One turn of the intake.  false: nothing waited and the stream goes on — the fiber has yielded, the caller comes again.  `noun` is the
	// node's word for itself in the "Channel count changed" error.
	template <class Hold>
	bool take_in(Intake& in, Audio_stream& input_stream, const char* noun, const Hold& hold)
	{
		bool ended = false;
		const std::vector<Frame_ptr> batch = collect_batch(input_stream, in.held, &ended);
		in.at_end = batch.empty() && ended;
		if (batch.empty() && !ended)
		{
			nae_fiber::this_fiber::yield();
			return false;
		}
		if (batch.empty()) return true;
		const Frame_data* frame = batch.front()->data();
		if (in.ch == 0)
		{
			in.ch = frame->ch_layout.nb_channels;
			if (in.ch != 1 && in.ch != 2)
				throw infra::Processor::Runtime_error("Invalid channel count", "Only mono and stereo audio are supported.", infra::fmt("Got %d channels", in.ch));
			in.need = hold(frame);
		}
		else if (frame->ch_layout.nb_channels != in.ch)
			throw infra::Processor::Runtime_error("Channel count changed", infra::fmt("The %s runs one stream of a fixed channel count.", noun),
												  infra::fmt("Got %d channels after %d", frame->ch_layout.nb_channels, in.ch));
		for (const auto& f : batch)
		{
			in.shapes.push_back({f->data()->nb_samples, f->data()->sample_rate, f->data()->pts, f->data()->time_base});
			in.pending.push_back(f);
			in.pending_samples += (size_t)f->data()->nb_samples;
		}
		return true;
	}

	// The counterpart: n samples of interleaved f32 leave as packed float frames of the shapes at the front of the queue, as long as a whole
	// frame is there -> the samples that left
	inline size_t cut_and_push(std::deque<Shape>& shapes, const float* samples, size_t n, int ch, const Output_streams& output_stream, const std::atomic<bool>& stop_token)
	{
		size_t pos = 0;
		while (!shapes.empty() && !stop_token && n - pos >= (size_t)shapes.front().nb_samples)
		{
			const Shape s = shapes.front();
			shapes.pop_front();
			push_to_all(output_stream, make_f32_frame(samples + pos * ch, s.nb_samples, ch, s.sample_rate, s.pts, s.time_base), stop_token);
			pos += s.nb_samples;
		}
		return pos;
	}
}
