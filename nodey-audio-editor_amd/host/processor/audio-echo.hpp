// processor/audio-echo.hpp — a node the reference has no class for: a feedback delay with damped, optionally ping-pong repeats on the library's
// echo (nae_echo_*; DESIGN.md §3, "K16 echo").  Registered by infra::register_echo_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

#include <optional>

namespace processor
{
	// Registered as "audio_echo": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "delay_ms"        above 0: the delay of the left (or only) channel                       (default 350)
	//   "delay_ms_right"  above 0: the right channel's delay                                     (default: absent, the left delay)
	//   "feedback"        0 ... 0.95: what a repeat keeps of the one before                      (default 0.4)
	//   "ping_pong"       bool: each channel's loop listens to the other channel's line          (default false)
	//   "damp_hz"         0 (none) or 200 ... 20000: a low-pass in the loop                      (default 0)
	//   "lowcut_hz"       0 (none) or 20 ... 2000: a high-pass in the loop                       (default 0)
	//   "wet"             0 ... 1: the level of the repeats                                      (default 0.35)
	//   "dry"             0 ... 1: the level of the input                                        (default 1)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The parameters
	// are designed from the stream's sample rate when the first frame arrives (nae_echo_design); a delay under 1024 or above 1048576 samples
	// at that rate, or a corner at or above Nyquist, is a Runtime_error then.  The node delivers exactly the frames it received, as packed
	// float frames of their sizes, pts and time base, and flushes at the end of the stream: the repeats that would sound after it are dropped.
	// the keys above as a plain copyable record: the node is one
	struct Echo_settings
	{
		static constexpr double default_delay_ms = 350, default_feedback = 0.4, default_damp_hz = 0, default_lowcut_hz = 0, default_wet = 0.35,
								default_dry = 1;
		double delay_ms = default_delay_ms;
		std::optional<double> delay_ms_right;   // none: the left delay
		double feedback = default_feedback, damp_hz = default_damp_hz, lowcut_hz = default_lowcut_hz, wet = default_wet, dry = default_dry;
		bool ping_pong = false;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_echo : public infra::Processor, public Echo_settings
	{
	  public:

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;
		void deserialize(const Json::Value& value) override;
	};
}
