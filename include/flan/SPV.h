// flan/SPV.h -- the sliding-DFT phase vocoder (mirrors the reference's src/flan/SPV/SPV.h; Conversions/AudioSPV.cpp, SPV/SPV.cpp).
#pragma once
#include "flan/Function.h"
#include "flan/SPVBuffer.h"
#include "flan/defines.h"

namespace flan {

class Audio;

class SPV : public SPVBuffer
	{
public:
	SPV();
	SPV( SPVBuffer && other );
	explicit SPV( const Format & );
	SPV copy() const;

	/** AudioSPV.cpp:110-145: inverse phase vocoder per bin, sample = 2 sum_b (-1)^b m cos( phase ).  On the device (flanhip_spv_synthesize_dev). */
	Audio convert_to_audio( flan_CANCEL_ARG ) const;
	/** AudioSPV.cpp:147-150: convert_to_audio().convert_to_left_right() */
	Audio convert_to_lr_audio( flan_CANCEL_ARG ) const;

	/** SPV.cpp:21-38: every MF's f becomes mod( TF{ frame_to_time( frame ), f } ).  A constant Function runs on the device; a callable is
	 *  evaluated on the host copy, per MF, as the reference does. */
	SPV modify_frequency( const Function<TF, Frequency> & mod ) const;
	/** SPV.cpp:40-44: modify_frequency( tf.f * mod( tf ) ) */
	SPV repitch( const Function<TF, Frequency> & mod ) const;
	};

} // namespace flan
