// processor/audio-multiband.hpp — a node the reference has no class for: a multiband compressor on the library's crossover and per-band
// compressor (nae_mb_*; DESIGN.md §3, "K20 multiband").  Registered by infra::register_multiband_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-dynamics.hpp"

#include <vector>

namespace processor
{
	// Registered as "audio_multiband": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "crossovers"     array of 1 ... 3 ascending frequencies in Hz: two, three or four bands on fourth-order
	//                    Linkwitz-Riley crossovers whose bands add to a flat magnitude                         (default [120, 2500])
	//   "bands"          array of exactly crossovers + 1 objects, lowest band first; absent: every band at the defaults
	//   "lookahead_ms"   0 ... 20: one look-ahead for all bands; at most 1024 samples at the stream's rate     (default 0)
	//   "link_channels"  bool: one detector per band for both channels of a stereo stream                      (default true)
	// A band object takes "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms" and "makeup_db" with audio_dynamics' ranges and
	// defaults (audio-dynamics.hpp; the one list of fields in audio-effects.cpp), "mute": bool, the band is left out of the sum (muting all
	// bands but one is a solo), and "bypass": bool, the band passes its compressor by.
	// A value of the wrong type or outside its range, or an array of the wrong length: Runtime_error "Wrong field: <key>".  Defaults are not
	// written back.  The parameters are designed from the stream's sample rate on the first frame (nae_dyn_design per band, nae_mb_design); a
	// crossover at or above half that rate, or a look-ahead above 1024 samples at it, is a Runtime_error then.  The node delivers exactly the
	// frames it received, as packed float frames of their sizes, pts and time base.
	// the keys above as a plain copyable record: the node is one
	struct Multiband_settings
	{
		static constexpr size_t max_crossovers = 3;
		static constexpr double min_crossover_hz = 1.0, max_crossover_hz = 1.0e6, default_lookahead_ms = 0;
		// a band's compressor is a Dynamics_settings of which the band's six keys are read; its mode, look-ahead and link are not
		struct Band
		{
			Dynamics_settings dynamics;
			bool mute = false, bypass = false;
		};
		std::vector<double> crossovers = {120.0, 2500.0};
		std::vector<Band> bands = std::vector<Band>(3);   // always crossovers.size() + 1 of them
		double lookahead_ms = default_lookahead_ms;
		bool link_channels = true;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_multiband : public infra::Processor, public Multiband_settings
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
