// processor/audio-gate.hpp — a node the reference has no class for: a noise gate and downward expander on the library's gate
// (nae_gate_*; DESIGN.md §3, "K19 gate").  Registered by infra::register_gate_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_gate": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "mode"           "gate" | "expander": everything below the threshold goes down by the range,
	//                    or by (ratio - 1) dB for every dB it lies below                               (default "gate")
	//   "threshold_db"   -90 ... 0: the level at which the gate opens                                  (default -40)
	//   "hysteresis_db"  0 ... 24: the gate closes this far below the threshold, so a level that
	//                    hovers around it does not chatter                                             (default 3)
	//   "range_db"       0 ... 120: the deepest attenuation                                            (default 60)
	//   "ratio"          1 ... 100: the expander's ratio; the gate mode does not read it               (default 2)
	//   "attack_ms"      0 ... 500: how fast the gate opens                                            (default 1)
	//   "hold_ms"        0 ... 10000: how long it stays open behind the last level above the
	//                    closing threshold                                                             (default 50)
	//   "release_ms"     1 ... 5000: how fast it closes                                                (default 100)
	//   "lookahead_ms"   0 ... 20: the gate opens this long before the level rises, so an attack is
	//                    not cut; at most 1024 samples at the stream's sample rate                     (default 0)
	//   "link_channels"  bool: one decision for both channels of a stereo stream                       (default true)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The
	// parameters are designed from the stream's sample rate on the first frame; a look-ahead above 1024 samples at that rate is a
	// Runtime_error then.  The node delivers exactly the frames it received, as packed float frames of their sizes, pts and time base.
	// the keys above as a plain copyable record: the node is one
	struct Gate_settings
	{
		enum class Mode { Gate, Expander };
		static constexpr double default_threshold_db = -40, default_hysteresis_db = 3, default_range_db = 60, default_ratio = 2, default_attack_ms = 1,
								default_hold_ms = 50, default_release_ms = 100, default_lookahead_ms = 0;
		Mode mode = Mode::Gate;
		double threshold_db = default_threshold_db, hysteresis_db = default_hysteresis_db, range_db = default_range_db, ratio = default_ratio,
			   attack_ms = default_attack_ms, hold_ms = default_hold_ms, release_ms = default_release_ms, lookahead_ms = default_lookahead_ms;
		bool link_channels = true;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_gate : public infra::Processor, public Gate_settings
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
