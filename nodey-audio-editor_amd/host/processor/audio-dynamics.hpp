// processor/audio-dynamics.hpp — a node the reference has no class for: a compressor / look-ahead limiter on the library's dynamics processor
// (nae_dyn_*; DESIGN.md §3, "K12 dynamics").  Registered by infra::register_dynamics_processors().  Its process_payload stands in
// audio-effects.cpp, next to the equalizer node's: both run on the one loop that feeds a streaming handle and delivers its frames.
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_dynamics": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "mode"           "compressor" | "limiter"; a limiter has slope 1 and ignores "ratio"   (default "compressor")
	//   "threshold_db"   -60 ... 0                                                            (default -18)
	//   "ratio"          1 ... 100                                                            (default 4)
	//   "knee_db"        0 ... 24                                                             (default 6)
	//   "attack_ms"      0 ... 500                                                            (default 5)
	//   "release_ms"     1 ... 5000                                                           (default 100)
	//   "lookahead_ms"   0 ... 20                                                             (default 0)
	//   "makeup_db"      -24 ... 24                                                           (default 0)
	//   "link_channels"  bool: one detector for both channels of a stereo stream              (default true)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The parameters
	// are designed from the stream's sample rate when the first frame arrives (nae_dyn_design); a look-ahead of more than 1024 samples at
	// that rate is a Runtime_error then.  The node delivers exactly the frames it received, as packed float frames of their sizes, pts and
	// time base — the look-ahead is compensated — and flushes at the end of the stream.
	// the nine keys as a plain copyable record: the dynamics node is one, and the side-chain node (audio-sidechain.hpp) holds one
	struct Dynamics_settings
	{
		enum class Mode { Compressor = 0, Limiter };
		static constexpr double default_threshold_db = -18, default_ratio = 4, default_knee_db = 6, default_attack_ms = 5, default_release_ms = 100,
								default_lookahead_ms = 0, default_makeup_db = 0;
		Mode mode = Mode::Compressor;
		double threshold_db = default_threshold_db, ratio = default_ratio, knee_db = default_knee_db, attack_ms = default_attack_ms,
			   release_ms = default_release_ms, lookahead_ms = default_lookahead_ms, makeup_db = default_makeup_db;
		bool link_channels = true;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_dynamics : public infra::Processor, public Dynamics_settings
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
