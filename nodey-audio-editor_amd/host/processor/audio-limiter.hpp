// processor/audio-limiter.hpp — a node the reference has no class for: a true-peak look-ahead brickwall limiter on the library's limiter
// (nae_lim_*; DESIGN.md §3, "K22 limiter").  Registered by infra::register_limiter_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_limiter": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "ceiling_db"     -20 ... 0: no output sample lies above it                                     (default -1)
	//   "gain_db"        -24 ... 24: the drive in front of the limiter                                 (default 0)
	//   "release_ms"     1 ... 5000: how fast the gain comes back                                      (default 100)
	//   "lookahead_ms"   0 ... 20: the gain starts down this long before a peak and reaches its value
	//                    at the peak; at most 1018 samples at the stream's sample rate                 (default 1.5)
	//   "true_peak"      bool: the detector hears the 4x oversampled signal, so peaks between the
	//                    samples count                                                                 (default true)
	//   "link_channels"  bool: one gain for both channels of a stereo stream                           (default true)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The
	// parameters are designed from the stream's sample rate on the first frame; a look-ahead above 1018 samples at that rate is a
	// Runtime_error then.  The node delivers exactly the frames it received, as packed float frames of their sizes, pts and time base.
	// the keys above as a plain copyable record: the node is one
	struct Limiter_settings
	{
		static constexpr double default_ceiling_db = -1, default_gain_db = 0, default_release_ms = 100, default_lookahead_ms = 1.5;
		double ceiling_db = default_ceiling_db, gain_db = default_gain_db, release_ms = default_release_ms, lookahead_ms = default_lookahead_ms;
		bool true_peak = true, link_channels = true;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_limiter : public infra::Processor, public Limiter_settings
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
