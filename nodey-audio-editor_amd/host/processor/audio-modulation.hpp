// processor/audio-modulation.hpp — a node the reference has no class for: chorus, flanger and vibrato on the library's modulated delay
// (nae_mod_*; DESIGN.md §3, "K17 modulated delay").  Registered by infra::register_modulation_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_modulation": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "rate_hz"    0 ... 20: the LFO's rate; 0 is a fixed comb                                  (default 0.8)
	//   "delay_ms"   above 0: the centre delay                                                   (default 12)
	//   "depth_ms"   0 or more: the sweep's amplitude                                            (default 3)
	//   "feedback"   -0.95 ... 0.95: what the line takes back of the delayed signal              (default 0)
	//   "voices"     integer 1 ... 4: taps of the one LFO, spread evenly over its turn           (default 3)
	//   "spread"     0 ... 1: the right channel's LFO behind the left one's, in half turns       (default 0.5)
	//   "shape"      "sine" | "triangle"                                                         (default "sine")
	//   "wet"        0 ... 1: the level of the delayed signal                                    (default 0.5)
	//   "dry"        0 ... 1: the level of the input                                             (default 1)
	// The defaults are a chorus.  A flanger: delay_ms 3, depth_ms 2, rate_hz 0.25, feedback 0.7, voices 1, wet 0.7; a vibrato: delay_ms 5,
	// depth_ms 2, rate_hz 5, voices 1, spread 0, wet 1, dry 0.
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The parameters
	// are designed from the stream's sample rate when the first frame arrives (nae_mod_design); a delay range [delay - depth, delay + depth]
	// outside 2 ... 3070 samples at that rate is a Runtime_error then.  The node delivers exactly the frames it received, as packed float
	// frames of their sizes, pts and time base, and flushes at the end of the stream: what would sound after it is dropped.
	// the keys above as a plain copyable record: the node is one
	struct Modulation_settings
	{
		enum class Shape { Sine, Triangle };
		static constexpr double default_rate_hz = 0.8, default_delay_ms = 12, default_depth_ms = 3, default_feedback = 0, default_spread = 0.5,
								default_wet = 0.5, default_dry = 1;
		static constexpr int default_voices = 3;
		double rate_hz = default_rate_hz, delay_ms = default_delay_ms, depth_ms = default_depth_ms, feedback = default_feedback,
			   spread = default_spread, wet = default_wet, dry = default_dry;
		int voices = default_voices;
		Shape shape = Shape::Sine;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_modulation : public infra::Processor, public Modulation_settings
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
